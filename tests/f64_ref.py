"""Host reference of the float64 half step (wmf_half_step_f64: RecModel/wmf_model.py:242-309), row by row, in plain NumPy.

The CSR is read AS STORED: a stored zero is an entry (it contributes p = 1 to the right-hand side), a duplicated column is two
entries.  For a row u with entries e = (idx_e, c_e)

    A_u = G~ + lambda I + Y~_u^T diag(w) Y~_u,      b_u = Y~_u^T (w + 1),      x_u = A_u^-1 b_u

where Y~ is Y with column 0 read as 1 when there is a bias and w = c - Y[idx, 0] then (wmf_model.py:253-257, :279), w = c
otherwise.  G~, A_u and b_u are accumulated in np.longdouble (64-bit mantissa here); x_u is LAPACK's float64 solve of the
rounded system followed by three steps of iterative refinement whose residual is taken in np.longdouble against the
longdouble system.  A row without entries is exactly 0.

half_step_batched is the form for the large cases (grid caps): float64 BLAS sums and ONE batched np.linalg.solve over the
stacked systems, no refinement -- NumPy's own float64 answer.

Per row the reference also gives
    cond   cond_2(A_u)                                          (only when asked: an SVD per row)
    tau    sum_e |w_e| y~_e^T (G~ + lambda I)^-1 y~_e           (what csrc/wmf_iter64.hip compares with IT64_TAU)
    eta    ||A_u x - b_u|| / (||A_u||_F ||x|| + ||b_u||)        (normwise backward error of a given x, residual in longdouble)
"""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble
REFINE_STEPS = 3


def tilde(Y, bias):
    """(Y~, the fixed side's biases or None)."""
    Y = np.asarray(Y, dtype=np.float64)
    if not bias:
        return Y, None
    Yt = Y.copy()
    Yt[:, 0] = 1.0
    return Yt, Y[:, 0].copy()


def gramian(Yt, lam, precise=True):
    """G~ + lambda I; longdouble sums when precise."""
    f = Yt.shape[1]
    G = np.zeros((f, f), dtype=LD)
    for lo in range(0, Yt.shape[0], 4096):                        # slabs bound the temporary of einsum
        if precise:
            S = Yt[lo: lo + 4096].astype(LD)
            G += np.einsum("ei,ej->ij", S, S)
        else:                                                     # float64 BLAS within a slab, longdouble across slabs
            S = Yt[lo: lo + 4096]
            G += (S.T @ S).astype(LD)
    return G + LD(lam) * np.eye(f, dtype=LD)


def row_taus(Y, bias, lam, indptr, indices, values):
    """tau_u of every row in float64 (to place weights before the reference runs)."""
    Yt, col0 = tilde(Y, bias)
    Ginv = np.linalg.inv(gramian(Yt, lam, precise=False).astype(np.float64))
    idx = np.asarray(indices, dtype=np.int64)[: int(indptr[-1])]
    q = np.einsum("ei,ij,ej->e", Yt[idx], Ginv, Yt[idx])
    t = np.abs(weights(np.asarray(values)[: len(idx)], idx, col0)) * q
    return np.array([t[indptr[u]: indptr[u + 1]].sum() for u in range(len(indptr) - 1)])


def weights(values, idx, col0):
    """w of a row's entries: float64 arithmetic on the stored numbers, as the reference and the kernels do."""
    w = np.asarray(values, dtype=np.float64)
    return w - col0[idx] if col0 is not None else w


def row_system(G, Yt, col0, idx, values):
    """(A_u, b_u, w) of one row in longdouble."""
    w = weights(values, idx, col0)
    U = Yt[idx].astype(LD)
    wl = w.astype(LD)
    A = G + np.einsum("ei,ej->ij", U * wl[:, None], U)
    b = (wl + LD(1)) @ U
    return A, b, w


def solve_refined(A, b):
    """x of A x = b: float64 LU (getrf / getrs) of the rounded system, then REFINE_STEPS corrections with the residual of the
    longdouble system in longdouble.  Returns (x rounded to float64, NumPy's unrefined float64 solve)."""
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    lu = sla.lu_factor(A64, check_finite=False)
    x0 = sla.lu_solve(lu, b64, check_finite=False)
    x = x0.astype(LD)
    for _ in range(REFINE_STEPS):
        r = b - A @ x
        x = x + sla.lu_solve(lu, r.astype(np.float64), check_finite=False).astype(LD)
    return x.astype(np.float64), x0


def backward_error(A, b, x):
    """eta of x for the longdouble system (A, b)."""
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    r = A @ xl - b
    den = np.sqrt((A * A).sum()) * np.sqrt((xl * xl).sum()) + np.sqrt((b * b).sum())
    return float(np.sqrt((r * r).sum()) / den) if den > 0 else 0.0


def half_step(Y, bias, lam, indptr, indices, values, candidates=(), want_cond=False, rows=None, gram_precise=True):
    """The reference rows of a half step and what goes with them.

    candidates: solutions [n, f] of the same half step (the device's, under several switches); their eta comes back per row.
    rows: the rows to compute (default: all); the others stay 0 / nan.  want_cond: True, or "neg" for the rows with a weight
    below zero only.
    gram_precise=False: the Gramian of a very long fixed side by float64 BLAS on slabs of 4096 rows, summed in longdouble.
    Returns a dict: x [n, f]; x_numpy [n, f] (the unrefined float64 solve); tau, cond, eta_numpy [n]; eta [len(candidates), n];
    neg [n] (the row has a weight below zero); pd [n] (A_u is positive definite: what a Cholesky kernel can take); degree [n]."""
    Yt, col0 = tilde(Y, bias)
    f = Yt.shape[1]
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1
    G = gramian(Yt, lam, gram_precise)
    Ginv = np.linalg.inv(G.astype(np.float64))
    out = {"x": np.zeros((n, f)), "x_numpy": np.zeros((n, f)), "tau": np.zeros(n), "cond": np.full(n, np.nan),
           "eta_numpy": np.zeros(n), "eta": np.zeros((len(candidates), n)), "neg": np.zeros(n, dtype=bool),
           "pd": np.ones(n, dtype=bool), "degree": np.diff(indptr)}
    for u in (range(n) if rows is None else rows):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi == lo:
            continue
        idx = np.asarray(indices[lo:hi], dtype=np.int64)
        A, b, w = row_system(G, Yt, col0, idx, values[lo:hi])
        out["x"][u], out["x_numpy"][u] = solve_refined(A, b)
        Ui = Yt[idx]
        out["tau"][u] = float(np.abs(w) @ np.einsum("ei,ij,ej->e", Ui, Ginv, Ui))
        out["neg"][u] = bool((w < 0).any())
        if out["neg"][u]:                                         # (all weights >= 0: A_u >= G~ + lambda I is positive definite)
            out["pd"][u] = bool(np.linalg.eigvalsh(A.astype(np.float64))[0] > 0)
        out["eta_numpy"][u] = backward_error(A, b, out["x_numpy"][u])
        for c, X in enumerate(candidates):
            out["eta"][c, u] = backward_error(A, b, X[u]) if np.isfinite(X[u]).all() else np.inf
        if want_cond is True or (want_cond == "neg" and out["neg"][u]):
            out["cond"][u] = np.linalg.cond(A.astype(np.float64))
    return out


def half_step_batched(Y, bias, lam, indptr, indices, values, batch=4096):
    """NumPy's own float64 answer for many short rows at once: the systems of `batch` rows are stacked and handed to ONE
    np.linalg.solve (gesv per system).  Sums in float64, a row's entries in stored order."""
    Yt, col0 = tilde(Y, bias)
    f = Yt.shape[1]
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    G = gramian(Yt, lam, precise=False).astype(np.float64)
    deg = np.diff(indptr)
    X = np.zeros((n, f))
    for r0 in range(0, n, batch):
        r1 = min(n, r0 + batch)
        full = np.flatnonzero(deg[r0:r1] > 0)                       # (reduceat has no empty segments)
        if not full.size:
            continue
        lo, hi = int(indptr[r0]), int(indptr[r1])
        idx = indices[lo:hi]
        w = weights(values[lo:hi], idx, col0)
        U = Yt[idx]
        starts = indptr[r0:r1][full] - lo
        A = G + np.add.reduceat(U[:, :, None] * (U * w[:, None])[:, None, :], starts, axis=0)
        b = np.add.reduceat(U * (w + 1.0)[:, None], starts, axis=0)
        X[r0 + full] = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    return X


def row_errors(got, ref):
    """||got_u - ref_u|| / ||ref_u|| per row; a row whose reference is 0 must be 0 exactly (error 0, or inf)."""
    num = np.linalg.norm(got - ref, axis=1)
    den = np.linalg.norm(ref, axis=1)
    err = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    return np.where(np.isfinite(got).all(axis=1), err, np.inf)
