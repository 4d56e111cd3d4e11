"""Host references for wmf_explain_rows / WMF.explain, and the cases the CPU and GPU tests share.

``ref64``       the definition, row by row in float64: contrib(u, i, e) = (w_e + 1) y~_i^T A_u^-1 y~_j with
                A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T (oracle/wmf_oracle.py::solve_row, RecModel/wmf_model.py:231-239 and
                :343-350) and total = sum_e contrib + beta_i.
``restated32``  the device kernel's algorithm in NumPy float32 (whitened gather, I + E_u entry by entry, right-looking Cholesky
                with reciprocal pivots, forward / backward substitution, t = W_white z, second pass), in the kernel's own
                summation orders with emulated fused multiply-adds.  Its error against ``ref64`` sets the gates.
The gate of a (row, target) pair: ``GATE_MARGIN`` x the pair error of ``restated32`` + ``GATE_FLOOR``, the pair error being
max_e |x - ref64| / max(max_e |ref64|, TINY) -- 4 x is the margin the row-solver tests give "the same algorithm in another
summation order", the floor is 8 float32 ulps (a contribution passes through the whitening, two substitutions, the
un-whitening and the final dot product: at least eight roundings even where the restatement happens to be exact).
"""
import functools
from fractions import Fraction

import numpy as np

GATE_MARGIN = 4.0
GATE_FLOOR = 8 * 2.0 ** -23
TINY = 1e-30
MAX_TARGETS = 16           # WMF_EXPLAIN_MAX_TARGETS
CHUNK = 8                  # stored entries the kernel gathers at a time
GRID_CAP = 1024            # workgroups of a launch: more rows than this take a second trip
N_ITEMS = 600
LAMBDA = 0.1


def tilde(Y, bias):
    """(y~, beta): the fixed side with column 0 read as 1, and its biases (zeros without a bias)."""
    Yt = np.array(Y, dtype=np.float64)
    beta = np.zeros(len(Yt))
    if bias:
        beta = Yt[:, 0].copy()
        Yt[:, 0] = 1.0
    return Yt, beta


def whitening(Y, bias, lam):
    """W_white = L^-T of G~ + lambda I = L L^T, float64 [f, f], upper triangular."""
    Yt, _ = tilde(Y, bias)
    L = np.linalg.cholesky(Yt.T @ Yt + lam * np.eye(Yt.shape[1]))
    return np.triu(np.linalg.inv(L).T)


def padded(M, ld):
    """float32 [rows, ld] with zero padding: the library's layout."""
    out = np.zeros((M.shape[0], ld), dtype=np.float32)
    out[:, :M.shape[1]] = M
    return out


def ref64(Y, bias, lam, indptr, indices, values, targets):
    """(contrib float64 [nnz, T], total float64 [n, T]); a -1 target gives zeros.  Y, values: the float32 data the device reads."""
    Yt, beta = tilde(Y, bias)
    G = Yt.T @ Yt + lam * np.eye(Yt.shape[1])
    n, T = targets.shape
    contrib = np.zeros((int(indptr[-1]), T))
    total = np.zeros((n, T))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        j = indices[lo:hi]
        w = np.asarray(values[lo:hi], dtype=np.float64) - beta[j]
        tg = targets[u]
        ok = tg >= 0
        U = Yt[j]
        A = G + U.T @ (U * w[:, None])
        c = (w + 1)[:, None] * (U @ np.linalg.solve(A, Yt[tg[ok]].T))
        contrib[lo:hi][:, ok] = c
        total[u, ok] = c.sum(axis=0) + beta[tg[ok]]
    return contrib, total


def _fma(a, b, c):
    """fl32(a b + c) as a fused multiply-add gives it: the product of two float32 is exact in float64, the sum is rounded to 53
    bits and then to 24 (a double rounding that differs from the fused result only on rare ties)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


_LANES = np.arange(16)


def _sum16(v):
    """The butterfly over the 16 lanes of a group (last axis): partners 8, 4, 2, 1 apart."""
    for o in (8, 4, 2, 1):
        v = v + v[..., _LANES ^ o]
    return v[..., 0]


def _whiten32(R, W):
    """q[:, b] = the fused sum over a = 0 .. b, in that order, of R[:, a] W[a, b]."""
    q = np.zeros_like(R)
    for a in range(R.shape[1]):
        q[:, a:] = _fma(R[:, a:a + 1], W[a:a + 1, a:], q[:, a:])
    return q


# ---- the row system of csrc/wmf_rowsystem.h in float32: what restated32 here, tests/foldin_ref.py and tests/posterior_ref.py share
def _prepared32(Y, bias, W32):
    """(y~, beta, W_white) in float32 as the kernels read them: column 0 as 1 with a bias, W_white's upper triangle."""
    f32 = np.float32
    f = Y.shape[1]
    Yt = np.array(Y, dtype=f32)
    beta = np.zeros(len(Yt), dtype=f32)
    if bias:
        beta = Yt[:, 0].copy()
        Yt[:, 0] = 1.0
    return Yt, beta, np.triu(np.asarray(W32, dtype=f32)[:, :f])


def _factor32(Yt, beta, W, j, vals, rhs=True):
    """rs_factor_row: (A, dinv, good, w) with L in the lower triangle of A[:f, :f] (the upper one is not the kernel's) and, with
    ``rhs``, c = L^-1 b in A[f, :f]; w the effective weights.  ``good`` is False where a pivot is not positive and finite."""
    f32 = np.float32
    f = Yt.shape[1]
    w = np.asarray(vals, dtype=f32) - beta[j]
    Q = _whiten32(Yt[j], W)
    A = np.zeros((f + rhs, f + rhs), dtype=f32)
    A[:f, :f] = np.eye(f, dtype=f32)
    for e in range(len(j)):
        A[:f, :f] = _fma((w[e] * Q[e])[:, None], Q[e][None, :], A[:f, :f])
        if rhs:
            A[f, :f] = _fma(w[e] + f32(1), Q[e], A[f, :f])
    dinv = np.zeros(f, dtype=f32)
    for k in range(f):
        p = A[k, k]
        if not (p > 0 and np.isfinite(p)):
            return A, dinv, False, w
        r = f32(1) / np.sqrt(p)
        dinv[k] = r
        col = A[k + 1:, k] * r
        A[k + 1:, k] = col
        A[k + 1:, k + 1:f] = _fma(-col[:, None], col[None, :f - k - 1], A[k + 1:, k + 1:f])
    return A, dinv, True, w


def _forward16(A, dinv, x):
    """rs_forward16: L z = q in place for the slots x [slots, f], a 16-lane group per slot."""
    for i in range(len(dinv)):
        s = np.zeros((len(x), 16), dtype=np.float32)
        for k0 in range(0, i, 16):
            cols = np.arange(k0, min(k0 + 16, i))
            s[:, :len(cols)] = _fma(A[i, cols][None, :], x[:, cols], s[:, :len(cols)])
        x[:, i] = (x[:, i] - _sum16(s)) * dinv[i]


def _backward(A, dinv, x):
    """rs_backward16 / rs_backward_wg (the same operations on every element): L^T g = x in place for x [slots, f]."""
    for k in range(len(dinv) - 1, -1, -1):
        zk = x[:, k] * dinv[k]
        x[:, :k] = _fma(-A[k, :k][None, :], zk[:, None], x[:, :k])
        x[:, k] = zk


def _unwhiten16(W, x):
    """rs_unwhiten: W g over b >= a for x [slots, f], lane g of a group over the columns a + g, a + g + 16, ..."""
    f = x.shape[1]
    t = np.zeros_like(x)
    for a in range(f):
        s = np.zeros((len(x), 16), dtype=np.float32)
        for b0 in range(a, f, 16):
            cols = np.arange(b0, min(b0 + 16, f))
            s[:, :len(cols)] = _fma(W[a, cols][None, :], x[:, cols], s[:, :len(cols)])
        t[:, a] = _sum16(s)
    return t


def restated32(Y, bias, W32, indptr, indices, values, targets):
    """The kernel's algorithm in float32, operation by operation and in the kernel's orders (csrc/wmf_explain.hip): sums over
    the 16 lanes of a group as strided partial sums and a butterfly, fused multiply-adds where the kernel fuses.  W32 float32
    [f, >= f] (the W_white the device is handed).  A row whose pivot is not positive and finite gives NaN."""
    f32 = np.float32
    f = Y.shape[1]
    Yt, beta, W = _prepared32(Y, bias, W32)
    n, T = targets.shape
    contrib = np.zeros((int(indptr[-1]), T), dtype=f32)
    total = np.zeros((n, T), dtype=f32)
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        j = indices[lo:hi]
        tg = targets[u]
        ok = tg >= 0
        if hi == lo:
            total[u, ok] = beta[tg[ok]]
            continue
        E, dinv, good, w = _factor32(Yt, beta, W, j, values[lo:hi], rhs=False)
        if not good:
            contrib[lo:hi][:, ok] = np.nan
            total[u, ok] = np.nan
            continue
        slots = np.nonzero(ok)[0]
        x = _whiten32(Yt[tg[ok]], W)                      # [slots, f]
        _forward16(E, dinv, x)
        _backward(E, dinv, x)
        t = _unwhiten16(W, x)
        s = np.zeros((hi - lo, len(slots), 16), dtype=f32)
        for a0 in range(0, f, 16):
            cols = np.arange(a0, min(a0 + 16, f))
            s[:, :, :len(cols)] = _fma(Yt[j][:, None, cols], t[None, :, cols], s[:, :, :len(cols)])
        c = ((w + f32(1))[:, None] * _sum16(s)).astype(f32)
        contrib[lo:hi][:, ok] = c
    total[:] = totals_in_order(contrib, Y, bias, indptr, targets)
    for u in range(n):
        if np.isnan(contrib[int(indptr[u]):int(indptr[u + 1])]).any():
            total[u, targets[u] >= 0] = np.nan
    return contrib, total


def pair_errors(x, ref, indptr):
    """[n, T]: max_e |x - ref| / max(max_e |ref|, TINY) of every (row, target) pair; 0 for an empty row."""
    n, T = len(indptr) - 1, ref.shape[1]
    out = np.zeros((n, T))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi > lo:
            d = np.abs(np.asarray(x[lo:hi], dtype=np.float64) - ref[lo:hi])
            out[u] = np.where(np.isnan(d).any(axis=0), np.inf, d.max(axis=0)) / np.maximum(np.abs(ref[lo:hi]).max(axis=0), TINY)
    return out


def totals_in_order(contrib32, Y, bias, indptr, targets):
    """out_total as documented: the row's float32 contributions added one by one in stored order from 0, then + beta_i; 0 for a
    -1 slot."""
    f32 = np.float32
    n, T = targets.shape
    beta = np.asarray(Y, dtype=f32)[:, 0] if bias else np.zeros(len(Y), dtype=f32)
    out = np.zeros((n, T), dtype=f32)
    for u in range(n):
        s = np.zeros(T, dtype=f32)
        for e in range(int(indptr[u]), int(indptr[u + 1])):
            s = s + contrib32[e]
        s = s + beta[np.maximum(targets[u], 0)]
        out[u] = np.where(targets[u] >= 0, s, f32(0))
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 4, 5, 16, 63, 64, 65, 100, 128, 129, 144, 192, 193, 256, 257, 260)      # tests/test_gpu_serving.py
LD_EXTRA = {5: 4, 64: 4, 100: 8, 129: 4, 257: 4, 260: 12}
WIDTH_CASES = [(f, b, 0) for f in WIDTHS for b in (0, 1) if f >= 2 or not b] + [(f, b, e) for f, e in LD_EXTRA.items() for b in (0, 1)]
# the kernel has one instantiation; its one storage edge is f = 31 / 32, where the 16 vectors t_i stop being larger than the
# packed triangle they replace (16 f against f (f + 1) / 2)
EDGE_CASES = [(f, b, 0) for f in (30, 31, 32) for b in (0, 1)]
FAMILY_WIDTHS = ((16, 0), (65, 1), (129, 1), (260, 0))
FAMILIES = ("gauss", "w1e3", "zeros", "dup", "eqbias", "neg")
T_CYCLE = (1, 2, MAX_TARGETS - 1, MAX_TARGETS)


def ld_for(f, extra=0):
    return (f + 3) // 4 * 4 + extra


def standard_degrees(f):
    """0 .. 3, the edges of the gather chunk, f - 1 .. f + 1, a row of several chunks; empty rows first, in the middle, last."""
    return [0, 1, 2, 3, 0, CHUNK - 1, CHUNK, CHUNK + 1, max(f - 1, 0), f, f + 1, 33, 0]


def _targets(rng, indptr, indices, m, T):
    """Items 0 and m - 1, an item of the row's own history, the same item twice, -1 slots, random items -- as T allows."""
    n = len(indptr) - 1
    tg = rng.integers(0, m, (n, T)).astype(np.int32)
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        want = [0, m - 1] if u % 2 == 0 else [m - 1]
        if hi > lo:
            want.insert(0, int(indices[lo + (u % (hi - lo))]))
        for k, v in enumerate(want[:T]):
            tg[u, k] = v
        if T >= 4:
            tg[u, T - 1] = tg[u, 0]                     # the same item twice
            tg[u, T - 2] = -1
        if T >= MAX_TARGETS - 1 and u % 3 == 0:
            tg[u, 5:9] = -1
    return tg


def make_case(name, f, extra, bias, family, degrees, T, seed, m=N_ITEMS):
    """A dict of host arrays: Y float32 [m, ld], W32 float32 [f, ld], indptr int64, indices int32, values float32 (confidences),
    targets int32 [n, T] -- what wmf_explain_rows is handed -- and f, ld, bias, lam."""
    rng = np.random.default_rng(seed)
    ld = ld_for(f, extra)
    Yf = (0.3 * rng.standard_normal((m, f)) if family == "gauss" else rng.random((m, f))).astype(np.float32)
    degrees = np.asarray(degrees, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    # distinct items within a row while the catalogue allows it (duplicates are their own family)
    indices = np.concatenate([rng.choice(m, d, replace=d > m) for d in degrees] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    nnz = len(indices)
    values = (10 * np.log1p(rng.integers(1, 6, nnz))).astype(np.float32)                  # the benchmark's confidences
    if family == "w1e3":
        values = rng.uniform(1.0, 1e3, nnz).astype(np.float32)
    elif family == "zeros":                             # stored zeros: effective weight 0, or -beta in (-1, 0] with a bias
        values[rng.random(nnz) < 0.5] = 0.0
    elif family == "dup":
        for u in range(len(degrees)):
            if degrees[u] >= 2:
                indices[indptr[u] + 1] = indices[indptr[u]]
    elif family == "eqbias":                            # value == bias exactly: effective weight 0
        hit = rng.random(nnz) < 0.5
        values[hit] = Yf[indices[hit], 0] if bias else 0.0
    elif family == "neg":                               # effective weights in (-1, 0): I + E_u stays positive definite
        values = (rng.uniform(-0.9, -0.1, nnz) + (Yf[indices, 0] if bias else 0.0)).astype(np.float32)
    W = whitening(Yf, bias, LAMBDA)
    return dict(name=name, f=f, ld=ld, bias=int(bias), lam=LAMBDA, m=m, Y=padded(Yf, ld), W32=padded(W, ld), indptr=indptr,
                indices=indices, values=values, targets=_targets(rng, indptr, indices, m, T), family=family)


def case_names():
    names = [f"width_f{f}_b{b}_x{e}" for f, b, e in WIDTH_CASES + EDGE_CASES]
    names += [f"{fam}_f{f}_b{b}" for f, b in FAMILY_WIDTHS for fam in FAMILIES]
    names += [f"targets_T{T}" for T in T_CYCLE]
    return names + ["long_row", "grid_cap"]


def inputs(name):
    """The host arrays of the case of that name (make_case), without references or gates."""
    kind = name.split("_")[0]
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    if kind == "width":
        f, b, e = (int(part[1:]) for part in name.split("_")[1:])
        k = (WIDTH_CASES + EDGE_CASES).index((f, b, e))
        c = make_case(name, f, e, b, "uniform", standard_degrees(f), T_CYCLE[k % 4], seed)
    elif kind == "targets":
        c = make_case(name, 100, 0, 0, "uniform", [0, 1, 5, 12, 40, 101], int(name[9:]), seed)
    elif name == "long_row":
        c = make_case(name, 65, 0, 1, "uniform", [2, 9000, 0, 3], 3, seed)
    elif name == "grid_cap":
        rng = np.random.default_rng(seed)
        c = make_case(name, 8, 0, 1, "uniform", rng.integers(0, 13, GRID_CAP + 6), 2, seed)
    else:
        f, b = (int(part[1:]) for part in name.split("_")[1:])
        c = make_case(name, f, 0, b, kind, [0, 1, 5, 12, 40, f + 1], 4, seed)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, with its float64 reference, the restatement's pair errors and the gates: built once, shared, never
    written (the arrays are read-only)."""
    c = inputs(name)
    Yf = c["Y"][:, :c["f"]]
    c["ref"], c["ref_total"] = ref64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], c["targets"])
    r32, _ = restated32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], c["targets"])
    c["restated_err"] = pair_errors(r32, c["ref"], c["indptr"])
    c["gate"] = GATE_MARGIN * c["restated_err"] + GATE_FLOOR
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


# ---- the exactly orthogonal catalogue -----------------------------------------------------------------------------------------
def orthogonal_case(f=12, m=40, seed=5):
    """Items are scaled unit vectors (no bias), so G~ and W_white are diagonal and whitened items on different axes are exactly
    orthogonal.  Returns the case and, per (entry, target) on the same axis, the closed form of the contribution evaluated with
    fractions.Fraction on the float32 inputs (Y, W32, values): (w + 1) s_i W_a (1 + sum_e' w_e' (s_e' W_a)^2)^-1 W_a s_j over
    the row's entries e' on that axis, without a rounding."""
    rng = np.random.default_rng(seed)
    axis = rng.integers(0, f, m)
    axis[:f] = np.arange(f)
    scale = rng.uniform(0.5, 2.0, m).astype(np.float32)
    Yf = np.zeros((m, f), dtype=np.float32)
    Yf[np.arange(m), axis] = scale
    ld = ld_for(f)
    W32 = padded(whitening(Yf, 0, LAMBDA), ld)
    degrees = np.array([1, 4, 9, 17, 30], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    indices = np.concatenate([rng.choice(m, d, replace=False) for d in degrees]).astype(np.int32)
    values = rng.uniform(1.0, 30.0, len(indices)).astype(np.float32)
    targets = rng.integers(0, m, (len(degrees), 6)).astype(np.int32)
    for u in range(len(degrees)):
        targets[u, 0] = indices[indptr[u]]
    exact = {}
    for u in range(len(degrees)):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        for t, i in enumerate(targets[u]):
            a = axis[i]
            Wa = Fraction(float(W32[a, a]))
            Eaa = 1 + sum(Fraction(float(values[e])) * (Fraction(float(scale[indices[e]])) * Wa) ** 2
                          for e in range(lo, hi) if axis[indices[e]] == a)
            for e in range(lo, hi):
                if axis[indices[e]] == a:
                    exact[(e, t)] = ((Fraction(float(values[e])) + 1) * Fraction(float(scale[i])) * Wa * Wa
                                     * Fraction(float(scale[indices[e]])) / Eaa)
    c = dict(name="orthogonal", f=f, ld=ld, bias=0, lam=LAMBDA, m=m, Y=padded(Yf, ld), W32=W32, indptr=indptr, indices=indices,
             values=values, targets=targets, axis=axis)
    return c, exact


def ulp_error(x, exact):
    """|x - exact| in units of the float32 ulp of exact (a Fraction, non-zero)."""
    mag = abs(exact)
    e = 0
    while Fraction(2) ** (e + 1) <= mag:
        e += 1
    while Fraction(2) ** e > mag:
        e -= 1
    return float(abs(Fraction(float(x)) - exact) / Fraction(2) ** (e - 23))


def orthogonal_ulp_bound():
    """2 x the worst ulp error of ``restated32`` against the closed form: the bound the device is held to."""
    c, exact = orthogonal_case()
    r32, _ = restated32(c["Y"][:, :c["f"]], 0, c["W32"], c["indptr"], c["indices"], c["values"], c["targets"])
    worst = max(ulp_error(r32[e, t], v) for (e, t), v in exact.items())
    return 2.0 * worst, worst
