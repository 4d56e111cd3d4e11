"""Host-side reference of the audit of a half step (include/wmf_hip.h, wmf_half_step_audit): the definitions in float64 NumPy, row
by row.  Nothing here touches a GPU; tests/test_audit_cpu.py checks it against a dense evaluation over all pairs and against the
reference's goldens.

For a half step that updates side R (rows x_u of X) against the fixed side F (rows of Y), with the CSR read as stored:
    y~_i = row i of F, column 0 read as 1 when bias;  beta_i = F[i, 0] when bias, else 0;  per entry (u, i, c): w = c - beta_i,
    s = x_u . y~_i;   S1 = sum (1 + w)(1 - s)^2, S2 = sum s^2, N = entries;
    r_u = (G~ + lam I) x_u + sum_e [w s - (w + 1)] y~_i,  b_u = sum_e (w + 1) y~_i,  a_u = sum_e |w| |y~_i|^2;
    L = <X^T X, G~>_F + S1 - S2 + lam |X|_F^2;   eta_u = |r_u| / ((|G~ + lam I|_F + a_u) |x_u| + |b_u|), 0 for a zero denominator.

EXACT inputs (integer factors, weights and dense term): every term is an integer; half_step_audit asserts that the sums of the
terms' magnitudes stay below 2^53, so every partial sum in ANY order is an integer float64 holds exactly and a device result has
to equal this one bit for bit."""
import numpy as np

LIMIT = 2.0 ** 53


def y_tilde(Y, bias):
    Yt = np.array(Y, dtype=np.float64)
    if bias:
        Yt[:, 0] = 1.0
    return Yt


def gram(Y, bias):
    """G~ = sum_i y~_i y~_i^T in float64: what wmf_gram(bias) returns."""
    Yt = y_tilde(Y, bias)
    return Yt.T @ Yt


def _all_integers(*arrays):
    return all(a is None or bool(np.all(np.asarray(a, dtype=np.float64) == np.rint(np.asarray(a, dtype=np.float64)))) for a in arrays)


def half_step_audit(X, Y, bias, indptr, indices, values, dense=None):
    """(sums float64 [3] = S1, S2, N;  rows float64 [n, 3] = |r_u|^2, |b_u|^2, a_u, or None without `dense` [n, f])."""
    X = np.asarray(X, dtype=np.float64)
    Yt = y_tilde(Y, bias)
    beta = np.asarray(Y, dtype=np.float64)[:, 0] if bias else np.zeros(len(Y))
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    n = len(indptr) - 1
    exact = _all_integers(X, Y, values[indptr[0]: indptr[-1]], dense)
    s1 = s2 = 0.0
    rows = np.zeros((n, 3)) if dense is not None else None
    bound_sums = 0.0
    for u in range(n):
        lo, hi = indptr[u], indptr[u + 1]
        idx = indices[lo:hi]
        Yu = Yt[idx]
        w = values[lo:hi] - beta[idx]
        s = Yu @ X[u]
        s1 += float(np.sum((1.0 + w) * (1.0 - s) ** 2))
        s2 += float(np.sum(s * s))
        if exact:
            s_abs = np.abs(Yu) @ np.abs(X[u])
            bound_sums += float(np.sum((1.0 + np.abs(w)) * (1.0 + s_abs) ** 2))
        if rows is not None:
            coef = w * s - (w + 1.0)
            r = np.asarray(dense[u], dtype=np.float64) + coef @ Yu
            b = (w + 1.0) @ Yu
            rows[u] = (r @ r, b @ b, np.sum(np.abs(w) * np.sum(Yu * Yu, axis=1)))
            if exact:
                r_abs = np.abs(np.asarray(dense[u], dtype=np.float64)) + (np.abs(w) * s_abs + np.abs(w) + 1.0) @ np.abs(Yu)
                assert max(r_abs @ r_abs, rows[u, 1], rows[u, 2]) < LIMIT, "integer inputs leave the exact range of float64"
    if exact:
        assert bound_sums < LIMIT, "integer inputs leave the exact range of float64"
    return np.array([s1, s2, float(indptr[-1] - indptr[0])]), rows


def eta_from_rows(rows, X, norm_a):
    """eta_u from {|r_u|^2, |b_u|^2, a_u}, |x_u| and |G~ + lam I|_F."""
    xn = np.linalg.norm(np.asarray(X, dtype=np.float64), axis=1)
    den = (norm_a + rows[:, 2]) * xn + np.sqrt(rows[:, 1])
    return np.where(den > 0, np.sqrt(rows[:, 0]) / np.where(den > 0, den, 1.0), 0.0)


def audit(X, Y, bias, lam, indptr, indices, values, rows=False):
    """What AlsEngine.audit(side, rows) returns, for the updated side X and the fixed side Y of one half step."""
    X = np.asarray(X, dtype=np.float64)
    f = X.shape[1]
    G = gram(Y, bias)
    A = G + lam * np.eye(f)
    sums, per_row = half_step_audit(X, Y, bias, indptr, indices, values, X @ A if rows else None)
    all_pairs = float(np.sum((X.T @ X) * G))
    reg = float(lam * np.sum(X * X))
    out = {"loss": all_pairs + sums[0] - sums[1] + reg, "all_pairs": all_pairs, "stored": float(sums[0] - sums[1]), "reg": reg,
           "n_stored": int(sums[2])}
    if rows:
        out["eta"] = eta_from_rows(per_row, X, np.linalg.norm(A))
    return out


def objective_dense(X, Y, bias, lam, C):
    """L by brute force over ALL (u, i) pairs, from a dense [n, m] array of SUMMED weights W (entries never stored: 0) and a dense
    count of stored entries per pair -- C = (weights [n, m, k] padded with NaN) is avoided: the caller passes the list of stored
    entries instead.  C: iterable of (u, i, c).  sum over pairs of s^2, plus per stored entry (1 + w)(1 - s)^2 - s^2."""
    X = np.asarray(X, dtype=np.float64)
    Yt = y_tilde(Y, bias)
    beta = np.asarray(Y, dtype=np.float64)[:, 0] if bias else np.zeros(len(Y))
    S = X @ Yt.T
    total = float(np.sum(S * S))
    for u, i, c in C:
        w = c - beta[i]
        total += (1.0 + w) * (1.0 - S[u, i]) ** 2 - S[u, i] ** 2
    return total + lam * float(np.sum(X * X))


def confidence(data, alpha=10, beta=1, pre_process_count='log'):
    """The confidence transform of RecModel/wmf_model.py:119-123 on a copy."""
    data = np.asarray(data)
    return alpha * np.log(1 + beta * data) if pre_process_count == 'log' else alpha * data
