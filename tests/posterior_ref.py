"""Host references for wmf_posterior_draw_rows / wmf_posterior_score_rows / wmf_posterior_noise and the model calls on them, and
the cases the CPU and GPU tests share.

``normal_h_int`` / ``normal_k``   the hash of the header in Python integers, and the same in uint64 NumPy: (k1, k2) of a triple.
``xi64``                          sqrt(-2 ln u1) cos(pi t) in float64.
``draws64``                       the definition of a draw given xi, row by row in float64: W L^-T (L^-1 b + sigma xi) with W the
                                  float64 whitening of the catalogue and L the Cholesky factor of I + E_u.
``scores64``                      mean = y~_i . x_u + beta_i with x_u the fold-in's definition, var = y~_i^T A_u^-1 y~_i by a dense
                                  solve with A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T.
``restated_draws32`` / ``restated_scores32``   the kernels' algorithm in NumPy float32, in the kernels' own summation orders with
                                  emulated fused multiply-adds (csrc/wmf_posterior.hip; the row system: tests/explain_ref.py).
                                  Their error sets the gates.
The gates are those of tests/foldin_ref.py: ``GATE_MARGIN`` x the error of the restatement on that element + ``GATE_FLOOR`` (8 ulps).
A draw's error is the fold-in's row error, max_a |x - ref| / max_a |ref|.  A variance is a sum of squares: its error is relative to
itself.  A mean is the dot product z . c (+ beta) and a float32 dot product's error is relative to sum |z_i c_i| <= |z| |c|, not to
the possibly cancelling sum: its error is taken relative to M = sqrt(var * c . c) + |beta_i|, where c . c = b^T (I + E_u)^-1 b =
rhs . x_u for rhs = sum_e (w_e + 1) y~_j.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import foldin_ref
import sample_ref
from explain_ref import (GATE_FLOOR, GATE_MARGIN, TINY, _backward, _factor32, _fma, _forward16, _prepared32, _sum16,  # noqa: F401
                         _unwhiten16, _whiten32, orthogonal_case, tilde, ulp_error, whitening)

MAX_DRAWS = 4096                   # WMF_POSTERIOR_MAX_DRAWS
MAX_TARGETS = 4096                 # WMF_POSTERIOR_MAX_TARGETS
MAX_F = 260                        # WMF_MAX_F
XI_BOUND = math.sqrt(48 * math.log(2))
GOLDEN_INT = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
CHI2_15_999 = 37.7                 # the 99.9 % point of chi-square with 15 degrees of freedom (37.697)


# ---- the noise ------------------------------------------------------------------------------------------------------------------
def mix_int(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def normal_key_int(draw, component):
    """The hash input of (draw, component) next to the row prefix: 2^32 (draw + 1) + component + 1."""
    return ((draw + 1) << 32) + component + 1


def normal_h_int(seed, stream, draw, component):
    a = mix_int(seed + GOLDEN_INT * (stream + 1))
    return mix_int(a + GOLDEN_INT * normal_key_int(draw, component))


def normal_k_int(seed, stream, draw, component):
    h = normal_h_int(seed, stream, draw, component)
    return h >> 41, (h >> 18) & 0x7FFFFF


def normal_k(seed, streams, draws, components):
    """(k1, k2), uint32 each, of every (stream, draw, component) triple, broadcast."""
    streams = np.asarray(streams, dtype=np.uint64)
    draws = np.asarray(draws, dtype=np.int64).astype(np.uint64)
    components = np.asarray(components, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        a = sample_ref.mix(np.uint64(seed) + sample_ref.GOLDEN * (streams + np.uint64(1)))
        key = ((draws + np.uint64(1)) << np.uint64(32)) + components + np.uint64(1)
        h = sample_ref.mix(a + sample_ref.GOLDEN * key)
    return (h >> np.uint64(41)).astype(np.uint32), ((h >> np.uint64(18)) & np.uint64(0x7FFFFF)).astype(np.uint32)


def xi64(k1, k2):
    u1 = (2.0 * np.asarray(k1, dtype=np.float64) + 1.0) * 2.0 ** -24
    t = (2.0 * np.asarray(k2, dtype=np.float64) + 1.0) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.pi * t)


def xi_block(seed, stream, n_draws, f):
    """float64 [n_draws, f]: the noise of one row."""
    k1, k2 = normal_k(seed, stream, np.arange(n_draws)[:, None], np.arange(f)[None, :])
    return xi64(k1, k2)


# ---- the definitions, float64 -----------------------------------------------------------------------------------------------------
def row_system(Y, bias, lam, indices, values):
    """(A_u, rhs) of one row from the definition: A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T, rhs = sum_e (w_e + 1) y~_j."""
    Yt, beta = tilde(Y, bias)
    j = np.asarray(indices)
    w = np.asarray(values, dtype=np.float64) - beta[j]
    U = Yt[j]
    return Yt.T @ Yt + lam * np.eye(Yt.shape[1]) + U.T @ (U * w[:, None]), (w + 1) @ U


def draws64(Y, bias, lam, indptr, indices, values, xi, sigma):
    """float64 [n, D, f]: x~ = W L^-T (L^-1 b + sigma xi) for xi [n, D, f]; an empty row has L = I and b = 0."""
    Yt, beta = tilde(Y, bias)
    W = whitening(Y, bias, lam)
    n, D, f = xi.shape
    out = np.zeros((n, D, f))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        j = indices[lo:hi]
        w = np.asarray(values[lo:hi], dtype=np.float64) - beta[j]
        Q = Yt[j] @ W
        L = np.linalg.cholesky(np.eye(f) + Q.T @ (Q * w[:, None]))
        c = np.linalg.solve(L, (w + 1) @ Q)
        out[u] = np.linalg.solve(L.T, (c[None, :] + sigma * xi[u]).T).T @ W.T
    return out


def scores64(Y, bias, lam, indptr, indices, values, targets):
    """(mean, var, M), float64 [n, T]: the definitions, and the magnitude the mean's error is relative to; a -1 slot gives zeros."""
    Yt, beta = tilde(Y, bias)
    n, T = targets.shape
    mean, var, M = (np.zeros((n, T)) for _ in range(3))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        A, rhs = row_system(Y, bias, lam, indices[lo:hi], values[lo:hi])
        x = np.linalg.solve(A, rhs)
        ok = targets[u] >= 0
        yi = Yt[targets[u][ok]]
        var[u, ok] = np.einsum("ta,at->t", yi, np.linalg.solve(A, yi.T))
        mean[u, ok] = yi @ x + beta[targets[u][ok]]
        M[u, ok] = np.sqrt(var[u, ok] * max(rhs @ x, 0.0)) + np.abs(beta[targets[u][ok]])
    return mean, var, M


# ---- the kernels' arithmetic, float32 -----------------------------------------------------------------------------------------------
def _lanes16(terms_a, terms_b, width):
    """sum16 over lanes g of the fused sums over i = g, g + 16, .. of a[.., i] b[.., i]: the kernels' dot product over `width`
    components."""
    s = np.zeros(terms_a.shape[:-1] + (16,), dtype=np.float32)
    for i0 in range(0, width, 16):
        cols = np.arange(i0, min(i0 + 16, width))
        s[..., :len(cols)] = _fma(terms_a[..., cols], terms_b[..., cols], s[..., :len(cols)])
    return _sum16(s)


def restated_draws32(Y, bias, W32, indptr, indices, values, xi32, sigma):
    """float32 [n, D, f] for xi32 float32 [n, D, f] (the device's own variates); a failed row gives NaN."""
    f32 = np.float32
    Yt, beta, W = _prepared32(Y, bias, W32)
    n, D, f = xi32.shape
    sigma = f32(sigma)
    out = np.zeros((n, D, f), dtype=f32)
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        empty = hi == lo
        if empty and sigma == 0:
            continue
        x = np.zeros((D, f), dtype=f32)
        if not empty:
            A, dinv, good, _ = _factor32(Yt, beta, W, indices[lo:hi], values[lo:hi])
            if not good:
                out[u] = np.nan
                continue
            x[:] = A[f, :f]
        if sigma != 0:
            x = _fma(sigma, xi32[u], x)
        if not empty:
            _backward(A, dinv, x)
        out[u] = _unwhiten16(W, x)
    return out


def restated_scores32(Y, bias, W32, indptr, indices, values, targets):
    """(mean, var), float32 [n, T]; a -1 slot gives zeros, a failed row NaN in its other slots."""
    f32 = np.float32
    Yt, beta, W = _prepared32(Y, bias, W32)
    f = Yt.shape[1]
    n, T = targets.shape
    mean, var = (np.zeros((n, T), dtype=f32) for _ in range(2))
    for u in range(n):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        ok = targets[u] >= 0
        tg = targets[u][ok]
        x = _whiten32(Yt[tg], W)
        if hi > lo:
            A, dinv, good, _ = _factor32(Yt, beta, W, indices[lo:hi], values[lo:hi])
            if not good:
                mean[u, ok] = var[u, ok] = np.nan
                continue
            _forward16(A, dinv, x)
            sm = _lanes16(x, np.broadcast_to(A[f, :f], x.shape), f)
        else:
            sm = np.zeros(len(tg), dtype=f32)
        var[u, ok] = _lanes16(x, x, f)
        mean[u, ok] = sm + beta[tg]
    return mean, var


# ---- errors and gates -------------------------------------------------------------------------------------------------------------
def draw_errors(x, ref):
    """[n, D]: the fold-in's row error of every draw."""
    n, D, f = ref.shape
    return foldin_ref.row_errors(np.asarray(x).reshape(n * D, f), ref.reshape(n * D, f)).reshape(n, D)


def score_errors(x, ref, scale):
    d = np.abs(np.asarray(x, dtype=np.float64) - ref)
    return np.where(np.isfinite(d), d, np.inf) / np.maximum(scale, TINY)


def gate_of(err):
    return GATE_MARGIN * err + GATE_FLOOR


def covariance_statistic(X, mean, cov):
    """N [tr(S C^-1) - log det(S C^-1) - f] for the sample covariance S of the rows of X around `mean`: twice the log-likelihood
    ratio of `cov` against the fitted covariance, chi-square with f (f + 1) / 2 degrees of freedom for draws from N(mean, cov)."""
    X = np.asarray(X, dtype=np.float64) - mean
    N, f = X.shape
    R = np.linalg.solve(cov, X.T @ X / N)
    return float(N * (np.trace(R) - np.linalg.slogdet(R)[1] - f))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
DRAW_WIDTHS = (1, 5, 30, 31, 32, 64, 129, 260)                     # the widths of the sigma = 0 identity and of the draws' gates
STAT_SEEDS = (11, 12, 13)
STAT_SIGMA = 0.75


def identity_case_names():
    """The fold-in's own cases at the widths of DRAW_WIDTHS, with and without biases, at both leading dimensions; the 9000-entry
    row and the 1030 rows."""
    names = [f"width_f{f}_b{b}_x{e}" for f, b, e in foldin_ref.WIDTH_CASES + foldin_ref.EDGE_CASES if f in DRAW_WIDTHS]
    return names + ["long_row", "grid_cap"]


def gated_case_names():
    """The cases the sigma > 0 draws and the scores are gated on: the widths with biases where the width allows (one layout each),
    and the six weight families at the fold-in's four family widths."""
    names = [f"width_f{f}_b{int(f > 1)}_x0" for f in DRAW_WIDTHS]
    return names + [f"{fam}_f{f}_b{b}" for f, b in foldin_ref.FAMILY_WIDTHS for fam in foldin_ref.FAMILIES]


def targets_for(c, T, seed=0):
    """int32 [n, T]: items 0 and m - 1, an item of the row's own history, the same item twice, -1 slots, random items -- as T allows."""
    rng = np.random.default_rng(1000 + seed + T)
    n, m = len(c["indptr"]) - 1, c["m"]
    tg = rng.integers(0, m, (n, T)).astype(np.int32)
    for u in range(n):
        lo, hi = int(c["indptr"][u]), int(c["indptr"][u + 1])
        want = [0, m - 1] + ([int(c["indices"][lo + u % (hi - lo)])] if hi > lo else [])
        for k, v in enumerate(want[:T]):
            tg[u, k] = v
        if T >= 5:
            tg[u, T - 1] = tg[u, 0]
            tg[u, T - 2] = -1
        if T >= 17 and u % 3 == 0:
            tg[u, 6:10] = -1
    return tg


def stat_case(bias):
    """f = 5, one history of 7 entries: the case of the draw statistics, with its float64 fold-in and posterior covariance."""
    c = dict(foldin_ref.make_case(f"stat_b{bias}", 5, 0, bias, "uniform", [7], 1, 77 + bias, m=200))
    Yf = c["Y"][:, :5]
    A, rhs = row_system(Yf, bias, c["lam"], c["indices"], c["values"])
    c["x"], c["cov"] = np.linalg.solve(A, rhs), STAT_SIGMA ** 2 * np.linalg.inv(A)
    return c


def reference_statistic(c, seed, n_draws=MAX_DRAWS):
    """The statistic of the float64 reference's own draws (the float64 xi of the hash) for stream 0 under `seed`."""
    Yf = c["Y"][:, :c["f"]]
    X = draws64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], xi_block(seed, 0, n_draws, c["f"])[None], STAT_SIGMA)[0]
    return covariance_statistic(X, c["x"], c["cov"])


def sqrt_fraction(q, bits=160):
    """sqrt of a positive Fraction to `bits` bits: as good as exact against a float32 ulp."""
    return Fraction(math.isqrt(q.numerator * (1 << 2 * bits) // q.denominator), 1 << bits)


@functools.lru_cache(maxsize=None)
def orthogonal_parts():
    """tests/explain_ref.py::orthogonal_case (items are scaled unit vectors, no bias: the row system is diagonal) and, per (row,
    axis), the exact rationals (W_a, L_aa^2, b_a, the history touches the axis) on the float32 inputs: L_aa^2 = 1 + W_a^2 sum_e w_e
    s_e^2 and b_a = W_a sum_e (w_e + 1) s_e over the row's entries on the axis.  On an axis a draw is W_a b_a / L_aa^2 + W_a sigma xi /
    L_aa, the variance of item i (s_i W_a)^2 / L_aa^2 and its mean s_i W_a b_a / L_aa^2, exactly 0 where the history misses the axis."""
    c, _ = orthogonal_case()
    parts = {}
    for u in range(len(c["indptr"]) - 1):
        entries = range(int(c["indptr"][u]), int(c["indptr"][u + 1]))
        for a in range(c["f"]):
            Wa = Fraction(float(c["W32"][a, a]))
            on = [(Fraction(float(c["values"][e])), Fraction(float(c["Y"][c["indices"][e], a]))) for e in entries
                  if c["axis"][c["indices"][e]] == a]
            parts[(u, a)] = (Wa, 1 + Wa * Wa * sum(w * s * s for w, s in on), Wa * sum((w + 1) * s for w, s in on), bool(on))
    return c, parts


def orthogonal_exact_draw(parts, u, a, sigma, xi):
    Wa, L2, ba, _ = parts[(u, a)]
    return Wa * ba / L2 + Wa * Fraction(float(sigma)) * Fraction(float(xi)) / sqrt_fraction(L2)


def orthogonal_exact_score(c, parts, u, i):
    """(mean, var) of item i for row u, exact."""
    a = int(c["axis"][i])
    Wa, L2, ba, _ = parts[(u, a)]
    s = Fraction(float(c["Y"][i, a]))
    return s * Wa * ba / L2, (s * Wa) ** 2 / L2
