"""Host references for wmf_foldin_rows / WMF.fold_in, and the cases the CPU and GPU tests share.

``ref64``       the definition, row by row in float64: x_u = A_u^-1 sum_e (w_e + 1) y~_j with A_u = G~ + lambda I +
                sum_e w_e y~_j y~_j^T (oracle/wmf_oracle.py::solve_row, RecModel/wmf_model.py:231-239 and :343-350); an empty
                row is zero.
``restated32``  the device kernel's algorithm in NumPy float32 (whitened gather, I + E_u and b entry by entry, right-looking
                Cholesky with reciprocal pivots that carries b as row f, backward substitution, x = W_white g), in the kernel's
                own summation orders with emulated fused multiply-adds.  Its error against ``ref64`` sets the gates.
The error of a row is max_a |x - ref64| / max(max_a |ref64|, TINY); the gate of a row is ``GATE_MARGIN`` x the row error of
``restated32`` + ``GATE_FLOOR``: the margin and the floor of tests/explain_ref.py, for its reasons (4 x for "the same algorithm
in another summation order"; a component passes through the whitening, the factorisation, a substitution and the un-whitening:
at least eight roundings even where the restatement happens to be exact).
The inputs are those of tests/explain_ref.py (``make_case``, the same names and seeds); the targets are ignored.
"""
import functools
from fractions import Fraction

import numpy as np

from explain_ref import (CHUNK, EDGE_CASES, FAMILIES, FAMILY_WIDTHS, GATE_FLOOR, GATE_MARGIN, GRID_CAP, LD_EXTRA, TINY,  # noqa: F401
                         WIDTH_CASES, WIDTHS, _backward, _factor32, _prepared32, _unwhiten16, ld_for, make_case, orthogonal_case, padded,
                         standard_degrees, tilde, ulp_error, whitening)


def ref64(Y, bias, lam, indptr, indices, values):
    """float64 [n, f]: the folded-in rows.  Y, values: the float32 data the device reads."""
    Yt, beta = tilde(Y, bias)
    G = Yt.T @ Yt + lam * np.eye(Yt.shape[1])
    n = len(indptr) - 1
    X = np.zeros((n, Yt.shape[1]))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi == lo:
            continue
        j = indices[lo:hi]
        w = np.asarray(values[lo:hi], dtype=np.float64) - beta[j]
        U = Yt[j]
        X[u] = np.linalg.solve(G + U.T @ (U * w[:, None]), (w + 1) @ U)
    return X


def restated32(Y, bias, W32, indptr, indices, values):
    """The kernel's algorithm in float32, operation by operation and in the kernel's orders (csrc/wmf_foldin.hip).  W32 float32
    [f, >= f] (the W_white the device is handed).  float32 [n, f]; a row whose pivot is not positive and finite gives NaN."""
    f = Y.shape[1]
    Yt, beta, W = _prepared32(Y, bias, W32)
    n = len(indptr) - 1
    X = np.zeros((n, f), dtype=np.float32)
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi == lo:
            continue
        A, dinv, good, _ = _factor32(Yt, beta, W, indices[lo:hi], values[lo:hi])
        if not good:
            X[u] = np.nan
            continue
        g = A[f:, :f].copy()                               # L^-1 b, the one right-hand side
        _backward(A, dinv, g)
        X[u] = _unwhiten16(W, g)[0]
    return X


def row_errors(x, ref):
    """[n]: max_a |x - ref| / max(max_a |ref|, TINY) of every row; inf where x is not finite."""
    d = np.abs(np.asarray(x, dtype=np.float64) - ref)
    bad = ~np.isfinite(d).all(axis=1)
    return np.where(bad, np.inf, np.where(bad[:, None], 0.0, d).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), TINY))


def gates(Y, bias, W32, indptr, indices, values, ref):
    """(gate [n], restated error [n]) of the rows against ``ref`` (their ref64)."""
    err = row_errors(restated32(Y, bias, W32, indptr, indices, values), ref)
    return GATE_MARGIN * err + GATE_FLOOR, err


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def case_names():
    names = [f"width_f{f}_b{b}_x{e}" for f, b, e in WIDTH_CASES + EDGE_CASES]
    names += [f"{fam}_f{f}_b{b}" for f, b in FAMILY_WIDTHS for fam in FAMILIES]
    return names + ["long_row", "grid_cap"]


def inputs(name):
    """The host arrays of the case of that name -- the inputs of tests/explain_ref.py::case, name for name, without the targets --
    without references or gates."""
    kind = name.split("_")[0]
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    if kind == "width":
        f, b, e = (int(part[1:]) for part in name.split("_")[1:])
        c = make_case(name, f, e, b, "uniform", standard_degrees(f), 1, seed)
    elif name == "long_row":
        c = make_case(name, 65, 0, 1, "uniform", [2, 9000, 0, 3], 3, seed)
    elif name == "grid_cap":
        rng = np.random.default_rng(seed)
        c = make_case(name, 8, 0, 1, "uniform", rng.integers(0, 13, GRID_CAP + 6), 2, seed)
    else:
        f, b = (int(part[1:]) for part in name.split("_")[1:])
        c = make_case(name, f, 0, b, kind, [0, 1, 5, 12, 40, f + 1], 4, seed)
    del c["targets"]
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name with its float64 reference, the restatement's row errors and the gates: built once, shared, never
    written (the arrays are read-only)."""
    c = inputs(name)
    Yf = c["Y"][:, :c["f"]]
    c["ref"] = ref64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"])
    c["gate"], c["restated_err"] = gates(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], c["ref"])
    c["live"] = np.diff(c["indptr"]) > 0
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


# ---- the exactly orthogonal catalogue -----------------------------------------------------------------------------------------
def orthogonal_exact():
    """tests/explain_ref.py::orthogonal_case (items are scaled unit vectors, no bias: G~ and W_white are diagonal) and, per (row,
    axis the row's history touches), the closed form of the folded-in component evaluated with fractions.Fraction on the
    float32 inputs: x_a = W_a^2 sum_e (w_e + 1) s_e / (1 + W_a^2 sum_e w_e s_e^2) over the row's entries on that axis, without a
    rounding.  The components on the other axes are exactly 0."""
    c, _ = orthogonal_case()
    exact = {}
    for u in range(len(c["indptr"]) - 1):
        entries = range(int(c["indptr"][u]), int(c["indptr"][u + 1]))
        for a in sorted({int(c["axis"][c["indices"][e]]) for e in entries}):
            Wa2 = Fraction(float(c["W32"][a, a])) ** 2
            on = [(Fraction(float(c["values"][e])), Fraction(float(c["Y"][c["indices"][e], a]))) for e in entries
                  if c["axis"][c["indices"][e]] == a]
            exact[(u, a)] = Wa2 * sum((w + 1) * s for w, s in on) / (1 + Wa2 * sum(w * s * s for w, s in on))
    return c, exact


def orthogonal_ulp_bound():
    """2 x the worst ulp error of ``restated32`` against the closed form: the bound the device is held to."""
    c, exact = orthogonal_exact()
    r32 = restated32(c["Y"][:, :c["f"]], 0, c["W32"], c["indptr"], c["indices"], c["values"])
    worst = max(ulp_error(r32[u, a], v) for (u, a), v in exact.items())
    return 2.0 * worst, worst
