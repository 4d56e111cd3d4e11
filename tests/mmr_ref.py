"""Host-side reference of the diversified top-n (include/wmf_hip.h, wmf_rerank_mmr and wmf_intra_list_similarity), in plain NumPy.
Nothing here touches a GPU: tests/test_mmr_ref_cpu.py checks it against a brute-force restatement.

Three forms of the one definition:
  * 'int'  -- int64 arithmetic for integer factors, integer relevances and lambda a multiple of 1/4, the dot metric: 4 v is an
              integer, nothing is rounded anywhere (mmr_greedy_int).
  * 'f32'  -- the header's float32 operations one by one (mmr_greedy with dtype float32).  It takes the dot as the float32 value of
              the exact sum, so it is the device's arithmetic only where that sum is exact in float32 in any order: the EXACT class
              of tests/serving_ref.py, and pow4_items below for the cosine (inverse norms that are powers of two).  On such inputs
              every later operation is exact as well, so the greedy sequence is forced and the device has to match bit for bit.
  * 'f64'  -- float64 throughout on the float32 inputs as given (mmr_greedy with dtype float64): what the ROUNDED class is held
              to, step by step, within v_bound (step_shortfalls)."""
import numpy as np

import serving_ref
import similar_ref

U32 = serving_ref.U32
LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)


# ---------------------------------------------------------------------------------------------------------------- inputs
def exact_items(n, f, seed):
    """The EXACT class of tests/serving_ref.py: integers in -3 .. 3 (the bias column too), a few all-zero rows."""
    return serving_ref.exact_factors(n, f, seed)


def pow4_items(n, f, bias, seed):
    """[n, f] float32 whose feature rows have 4^a entries of +-2^e (a <= 3, e in {0, 1}) and zeros elsewhere: the squared norm is
    the power of four 4^(a + e), the inverse norm a power of two, every dot a small integer, every cosine a dyadic number of a few
    bits.  Row n // 2 has no features at all (inverse norm 0).  The bias column holds integers in -3 .. 3."""
    rng = np.random.default_rng(seed)
    nf = f - int(bias)
    A = np.zeros((n, f), dtype=np.float32)
    a_max = max(a for a in range(4) if 4 ** a <= nf)
    for i in range(n):
        k = 4 ** int(rng.integers(0, a_max + 1))
        cols = rng.choice(nf, k, replace=False) + int(bias)
        A[i, cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), k) * np.float32(2.0 ** int(rng.integers(0, 2)))
    if n >= 4:
        A[n // 2] = 0
    if bias:
        A[:, 0] = rng.integers(-3, 4, n)
    return A


# ------------------------------------------------------------------------------------------------------------ similarity
class RowSims:
    """sim(j, s) among the candidates `ids` of one row, by position: column(p)[j] = sim(j, p).  F [n_items, f] unpadded."""

    def __init__(self, F, bias, ids, cosine, mode):
        assert mode in ("int", "f32", "f64") and not (mode == "int" and cosine)
        ids = np.asarray(ids, dtype=np.int64)
        X = np.asarray(F)[ids][:, int(bias):]
        self.X = np.rint(X).astype(np.int64) if mode == "int" else X.astype(np.float64)
        self.mode, self.cosine, self.inv = mode, bool(cosine), None
        if cosine:
            self.inv = (similar_ref.inv_norms_ref(F, bias) if mode == "f32" else similar_ref.inv_norms_f64(F, bias))[ids]

    def column(self, p):
        d = self.X @ self.X[p]
        if self.mode == "int":
            return d
        if self.mode == "f32":
            d32 = d.astype(np.float32) + np.float32(0)            # (the device's sum starts at +0: a zero dot is +0)
            assert (d32.astype(np.float64) == d).all(), "the f32 form needs dots that float32 holds exactly"
            return (d32 * self.inv) * self.inv[p] if self.cosine else d32
        return d * self.inv * self.inv[p] if self.cosine else d

    def matrix(self):
        """[c, c]: entry (j, p) = sim(j, p)."""
        c = len(self.X)
        return np.stack([self.column(p) for p in range(c)], axis=1) if c else np.zeros((0, 0))


# ------------------------------------------------------------------------------------------------------ greedy selection
def _first_max(v, taken):
    """The remaining position with the largest v; equal values (-0.0 == +0.0) go to the lower position."""
    rest = np.flatnonzero(~taken)
    return int(rest[np.argmax(v[rest])])


def mmr_greedy(r, column, lam, topn, dtype=np.float32):
    """(positions, v they were picked with): the header's selection in `dtype` operations, each rounded once.  `column(p)`: the
    sims of every candidate to candidate p.  lam is rounded to float32 first, as the C argument is."""
    r = np.asarray(r, dtype=dtype)
    c = len(r)
    lam_t = dtype(np.float32(lam))
    mu = dtype(1) - lam_t
    a = lam_t * r
    taken = np.zeros(c, dtype=bool)
    picks, values, m = [], [], None
    for t in range(min(int(topn), c)):
        if t == 0:
            v = a
        else:
            s = np.asarray(column(picks[-1]), dtype=dtype)
            m = s if t == 1 else np.where(s > m, s, m)
            v = a - mu * m
        p = _first_max(v, taken)
        picks.append(p)
        values.append(v[p])
        taken[p] = True
    return np.array(picks, dtype=np.int64), np.array(values, dtype=dtype)


def mmr_greedy_int(r, column, lam4, topn):
    """The same in int64: integer relevances, integer sims, lambda = lam4 / 4.  Returns (positions, 4 v)."""
    r = np.rint(np.asarray(r)).astype(np.int64)
    c, lam4 = len(r), int(lam4)
    taken = np.zeros(c, dtype=bool)
    picks, values, m = [], [], None
    for t in range(min(int(topn), c)):
        if t == 0:
            v = lam4 * r
        else:
            s = np.asarray(column(picks[-1]), dtype=np.int64)
            m = s if t == 1 else np.maximum(s, m)
            v = lam4 * r - (4 - lam4) * m
        p = _first_max(v, taken)
        picks.append(p)
        values.append(v[p])
        taken[p] = True
    return np.array(picks, dtype=np.int64), np.array(values, dtype=np.int64)


def padded_outputs(ids, r, picks, values, topn):
    """(out_items int32, out_scores float32, out_marginal float32) of one row as the header pads them."""
    k = len(picks)
    items = np.full(topn, -1, dtype=np.int32)
    scores = np.full(topn, -np.inf, dtype=np.float32)
    marg = np.full(topn, -np.inf, dtype=np.float32)
    items[:k] = np.asarray(ids)[picks]
    scores[:k] = np.asarray(r, dtype=np.float32)[picks]
    marg[:k] = np.asarray(values, dtype=np.float32)
    return items, scores, marg


# --------------------------------------------------------------------------------------------------- the ROUNDED class
def sim_bounds(F, bias, ids, picks, cosine):
    """(sim64, B) [c, len(picks)]: the float64 similarity of every candidate to every pick and the bound on the device's float32
    value of it: B' of tests/similar_ref.py for the dot (2 (nf + 2) 2^-24 sum |x y|, any order of summation), B_cos for the cosine."""
    ids, picks = np.asarray(ids, dtype=np.int64), np.asarray(picks, dtype=np.int64)
    X = np.asarray(F)[ids][:, int(bias):].astype(np.float64)
    P = X[picks]
    d = X @ P.T
    b = 2.0 * (X.shape[1] + 2) * U32 * (np.abs(X) @ np.abs(P).T)
    if not cosine:
        return d, b
    inv = similar_ref.inv_norms_f64(F, bias)[ids]
    cos = d * inv[:, None] * inv[picks][None, :]
    return cos, b * inv[:, None] * inv[picks][None, :] + 6.0 * U32 * np.abs(cos)


def v_bound(lam, r, m, bm):
    """E: the bound on |v_device - v64| of one candidate.  v_device = fl(fl(lam r) - fl(mu^ m^)) with mu^ = fl(1 - lam) and
    |m^ - m| <= bm (the max of computed sims is within the largest of their bounds of the max of the true ones).  The first term
    carries two relative errors of 2^-24 (its product, the subtraction), the second three (mu^, its product, the subtraction) on
    mu (|m| + bm); four on each covers them with the second-order terms.  Derived, not measured."""
    lam = float(np.float32(lam))
    mu = 1.0 - lam
    return mu * bm + 4.0 * U32 * (np.abs(lam * r) + mu * (np.abs(m) + bm))


def step_shortfalls(F, bias, ids, r, picks, lam, cosine):
    """For a device's own pick sequence: per step t (shortfall_t, E_t).  Given the prefix picks[:t], v64 of every remaining
    candidate; shortfall_t = max v64 - v64[picks[t]] (0 where the pick is the float64 argmax) and E_t = the largest v_bound among
    the remaining candidates.  The device may fall short by at most 2 E_t: its own v of the pick was the largest it computed."""
    r = np.asarray(r, dtype=np.float64)
    picks = np.asarray(picks, dtype=np.int64)
    lam64 = float(np.float32(lam))
    mu = 1.0 - lam64
    sim, bnd = sim_bounds(F, bias, ids, picks, cosine)
    taken = np.zeros(len(r), dtype=bool)
    out = []
    for t, p in enumerate(picks):
        assert not taken[p], "a position was picked twice"
        if t == 0:
            m, bm = np.zeros(len(r)), np.zeros(len(r))
        else:
            m, bm = sim[:, :t].max(axis=1), bnd[:, :t].max(axis=1)
        v = lam64 * r - mu * m
        e = v_bound(lam, r, m, bm)
        rest = ~taken
        out.append((float(v[rest].max() - v[p]), float(e[rest].max())))
        taken[p] = True
    return out


# --------------------------------------------------------------------------------------------------- intra-list similarity
def ils_ref(sims, n):
    """(mean float32, max float32) of a list of n entries in the header's order: S_j = the float64 sum of sim(j, i) over
    i = 0 .. j - 1 in that order, the total over j ascending, divided by n (n - 1) / 2 in float64 and rounded once.  `sims`: a
    RowSims over the list."""
    if n < 2:
        return np.float32(0), np.float32(-np.inf)
    M = sims.matrix()
    total, top = 0.0, -np.inf
    for j in range(1, n):
        s = 0.0
        for i in range(j):
            s += float(M[j, i])
            if M[j, i] > top:
                top = M[j, i]
        total += s
    return np.float32(total / (n * (n - 1) // 2)), np.float32(top)


def ils_bounds(F, bias, ids, cosine):
    """(mean64, bound on the mean, max64, bound on the max) of one list: the pairs' similarity bounds averaged, plus the rounding of
    the float64 sums and of the result (2 x 2^-24 |mean|); the largest pair bound for the max."""
    n = len(ids)
    sim, bnd = sim_bounds(F, bias, ids, np.arange(n), cosine)
    lower = np.tril_indices(n, -1)
    mean = float(sim[lower].mean())
    return mean, float(bnd[lower].mean()) + 2.0 * U32 * abs(mean), float(sim[lower].max()), float(bnd[lower].max())
