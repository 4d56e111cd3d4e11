"""Host-side references for the scoring, ranking and evaluation entry points (tests/test_gpu_serving.py), in plain NumPy.

Two input classes, as in tests/test_gpu_dense.py:
  * EXACT   -- factor entries are integers in -3 .. 3 (the bias column too): |score| <= 9 * 260 < 2^24, so every product and
               every partial sum is an integer float32 holds exactly, in any order of summation.  The reference is int64 and the
               device has to match it bit for bit; equal scores are real ties.
  * ROUNDED -- standard-normal float32 entries; the reference is float64 arithmetic on those float32 numbers and the device is
               held to score_bound().
Nothing here touches a GPU: tests/test_serving_ref_cpu.py checks these functions against the oracle."""
import numpy as np

U32 = 2.0 ** -24                                                  # unit roundoff of float32
WMF_MAX_F = 260


# ---------------------------------------------------------------------------------------------------------------- inputs
def exact_factors(n, f, seed):
    """[n, f] float32 of integers in -3 .. 3; a few all-zero rows, so that score 0 is common."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, (n, f)).astype(np.float32)
    if n >= 8:
        A[rng.choice(n, n // 8, replace=False)] = 0
    return A


def rounded_factors(n, f, seed):
    return np.random.default_rng(seed).standard_normal((n, f)).astype(np.float32)


def padded(A, ld, dtype=np.float32):
    """[n, ld]: A in the leading columns, zero padding columns (include/wmf_hip.h, conventions)."""
    P = np.zeros((A.shape[0], ld), dtype=dtype)
    P[:, :A.shape[1]] = A
    return P


# ---------------------------------------------------------------------------------------------------------------- scores
def _split(A, bias):
    return (A[:, 1:], A[:, 0]) if bias else (A, None)


def scores_int(Uf, If, users, items, bias):
    """int64 predict(users[p], items[p]) of EXACT-class factors (RecModel/wmf_model.py:205-211); one side may have length 1."""
    Ub, u0 = _split(np.rint(Uf).astype(np.int64), bias)
    Ib, i0 = _split(np.rint(If).astype(np.int64), bias)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    s = (Ub[users] * Ib[items]).sum(axis=1)
    return s + u0[users] + i0[items] if bias else s


def score_matrix_int(Uf, If, users, items, bias):
    """int64 [len(users), len(items)] score matrix of EXACT-class factors."""
    Ub, u0 = _split(np.rint(Uf).astype(np.int64), bias)
    Ib, i0 = _split(np.rint(If).astype(np.int64), bias)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    S = Ub[users] @ Ib[items].T
    return S + u0[users][:, None] + i0[items][None, :] if bias else S


def scores_f64(Uf, If, users, items, bias):
    """float64 predict on the float32 factors as given (what oracle.predict computes on float64 copies)."""
    Ub, u0 = _split(Uf.astype(np.float64), bias)
    Ib, i0 = _split(If.astype(np.float64), bias)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    s = (Ub[users] * Ib[items]).sum(axis=1)
    return s + u0[users] + i0[items] if bias else s


def score_bound(Uf, If, users, items, bias):
    """B(u, i) = 2 (f + 2) 2^-24 (sum_c |x_uc y_ic| + |x_u0| + |y_i0|): the any-order float32 summation bound gamma_f ~ f u over
    the absolute terms of the score (the products, and for a bias model the two biases, which enter as themselves), doubled
    because an MFMA's internal accumulation does not promise one rounding per addition.  Derived, not measured."""
    f = Uf.shape[1]
    Ub, u0 = _split(np.abs(Uf.astype(np.float64)), bias)
    Ib, i0 = _split(np.abs(If.astype(np.float64)), bias)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    mass = (Ub[users] * Ib[items]).sum(axis=1)
    if bias:
        mass = mass + u0[users] + i0[items]
    return 2.0 * (f + 2) * U32 * mass


# --------------------------------------------------------------------------------------------------------------- ranking
def stable_topn(scores, topn):
    """Positions of the topn best of `scores`, best first, equal scores in position order: the order both rank entry points
    promise (include/wmf_hip.h, wmf_rank_topn).  No NaNs."""
    scores = np.asarray(scores)
    n, topn = len(scores), int(topn)
    if 0 < topn and 4 * topn < n:                                 # only what reaches the cut is sorted; same result
        cut = np.partition(scores, n - topn)[n - topn]
        keep = np.flatnonzero(scores >= cut)
        return keep[_descending_stable(scores[keep])[:topn]]
    return _descending_stable(scores)[:topn]


def _descending_stable(scores):
    if scores.dtype.kind == "f":                                  # -0.0 == 0.0 and the infinities negate without trouble
        return np.argsort(-scores, kind="stable")
    return np.argsort(-scores.astype(np.int64), kind="stable")


def rank_key(scores):
    """The order-preserving uint32 key of a float32 score that the top-n select builds its 4096-bin histogram on (bin =
    key >> 20, 16 bins to a group; csrc/wmf_rank.hip)."""
    u = np.asarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# score levels of the histogram-boundary case (f = 1, user factor 1.0: score = item value)
HIST_VALUES = (-np.inf, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.0 + 2.0 ** -10, 1.125, 1.25, 2.0, 3e38, np.inf)


def hist_case(seed):
    """(values float32 shuffled, levels, counts): every level of HIST_VALUES between 1 and 40 times."""
    rng = np.random.default_rng(seed)
    levels = np.array(HIST_VALUES, dtype=np.float32)
    counts = rng.integers(1, 41, len(levels))
    counts[[0, 6, 12]] = (1, 40, 1)                               # both ends of the range occur
    values = np.repeat(levels, counts)
    rng.shuffle(values)
    return values, levels, counts


def hist_bin_properties(levels):
    """Which of the select's situations a set of score levels produces: two levels in one bin, two occupied bins in one 16-bin
    group, bins in different groups, a bin in group 0."""
    bins = (rank_key(np.asarray(levels, dtype=np.float32)) >> 20).astype(np.int64)
    occupied = np.unique(bins)
    groups = occupied >> 4
    return {
        "two_values_in_one_bin": len(occupied) < len(np.unique(np.asarray(levels, dtype=np.float32))),
        "two_bins_in_one_group": len(np.unique(groups)) < len(occupied),
        "different_groups": len(np.unique(groups)) > 1,
        "bin_in_group_0": bool((groups == 0).any()),
    }


# ------------------------------------------------------------------------------------------------------------ hit counts
def hit_counts(s_true, s_cand, slot, topn):
    """include/wmf_hip.h, wmf_hit_counts: hits[t] = number of test entries p for which fewer than topn[t] of the OTHER
    candidates of its row score strictly higher.  s_true [n_pairs], s_cand [n_pairs, n_cand] (scores of pair p's user against
    its candidate row), slot [n_pairs] (the position of that row that stands for the test item).  A tie is not higher."""
    s_true, s_cand = np.asarray(s_true), np.asarray(s_cand)
    n_pairs, n_cand = s_cand.shape if s_cand.ndim == 2 else (0, 0)
    topn = np.asarray(topn, dtype=np.int64)
    if n_pairs == 0:
        return np.zeros(len(topn), dtype=np.int64)
    other = np.arange(n_cand)[None, :] != np.asarray(slot)[:, None]
    higher = ((s_cand > s_true[:, None]) & other).sum(axis=1)
    return (higher[:, None] < topn[None, :]).sum(axis=0).astype(np.int64)


# -------------------------------------------------------------------------------------------------------------- eval sums
def eval_sums(scores, values):
    """RecModel.eval_prec's sums (base_model.py:163-176) over stored entries: (sum (v - s)^2, sum |v - s|, count) over the
    entries with v != 0 (stored 0.0 and -0.0 are skipped).  int64 scores and integer values give exact int64 sums."""
    values = np.asarray(values)
    keep = values != 0
    if np.asarray(scores).dtype.kind == "i":
        e = np.rint(values[keep]).astype(np.int64) - np.asarray(scores)[keep]
        return int((e * e).sum()), int(np.abs(e).sum()), int(keep.sum())
    e = values[keep].astype(np.float64) - np.asarray(scores, dtype=np.float64)[keep]
    return float((e * e).sum()), float(np.abs(e).sum()), int(keep.sum())


def csr_rows(indptr):
    """Row number of every stored entry."""
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
