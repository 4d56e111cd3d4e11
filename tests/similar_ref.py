"""Host-side reference of the neighbours in factor space (include/wmf_hip.h, wmf_row_inv_norms and wmf_similar_topn), in plain
NumPy on tests/serving_ref.py and tests/recommend_ref.py.  Nothing here touches a GPU: tests/test_similar_cpu.py checks it against a
brute-force float64 cosine.

The features of a row are its columns [bias, f): the bias column of a bias model is sliced off and serving_ref is called with
bias = 0.  EXACT-class dots are int64 and exact in float32; the two float32 multiplications of the header are then repeated in NumPy
float32 arithmetic (scale_f32), each rounded once, so the device has to match bit for bit."""
import numpy as np

import recommend_ref
import serving_ref

U32 = serving_ref.U32


def inv_norms_ref(M, bias):
    """float32 [n]: 1 / sqrt(S_i), S_i the float64 sum of the squared features of row i of M [n, f]; 0 where S_i == 0 or the
    quotient is not a finite float32."""
    S = (np.asarray(M)[:, int(bias):].astype(np.float64) ** 2).sum(axis=1)
    with np.errstate(divide="ignore", over="ignore"):
        r = (1.0 / np.sqrt(S)).astype(np.float32)
    r[~np.isfinite(r) | (S == 0)] = 0
    return r


def _features(Qf, Cf, bias):
    return Qf[:, int(bias):], Cf[:, int(bias):]


def dot_matrix_int(Qf, Cf, q_rows, c_rows, bias):
    """int64 [len(q_rows), len(c_rows)] feature dot products of EXACT-class factors."""
    return serving_ref.score_matrix_int(*_features(Qf, Cf, bias), q_rows, c_rows, 0)


def dot_matrix_f64(Qf, Cf, q_rows, c_rows, bias):
    """float64 feature dot products of the float32 factors as given."""
    Q, C = _features(Qf, Cf, bias)
    return Q[np.asarray(q_rows, dtype=np.int64)].astype(np.float64) @ C[np.asarray(c_rows, dtype=np.int64)].astype(np.float64).T


def dot_bound(Qf, Cf, q_rows, c_rows, bias):
    """B'(q, j): serving_ref.score_bound on the feature columns, as a matrix."""
    Q, C = _features(Qf, Cf, bias)
    qq, cc = np.repeat(np.asarray(q_rows, dtype=np.int64), len(c_rows)), np.tile(np.asarray(c_rows, dtype=np.int64), len(q_rows))
    return serving_ref.score_bound(Q, C, qq, cc, 0).reshape(len(q_rows), len(c_rows))


def scale_f32(d, sq, si):
    """(float32(d) * sq) * si in float32 operations, in that order: d [nq, nc], sq [nq] (the queries' scales), si [nc]."""
    d32 = np.asarray(d).astype(np.float32)
    return (d32 * np.asarray(sq, dtype=np.float32)[:, None]) * np.asarray(si, dtype=np.float32)[None, :]


def cosine_f64(d, sq, si):
    """float64 cosine of float64 dots d and the float64 feature norms behind sq, si given as 1 / norm (0 for a zero row)."""
    return np.asarray(d, dtype=np.float64) * np.asarray(sq, dtype=np.float64)[:, None] * np.asarray(si, dtype=np.float64)[None, :]


def inv_norms_f64(M, bias):
    """float64 1 / |features| (0 for a zero row): the scales of the float64 cosine the ROUNDED class is held to."""
    S = (np.asarray(M)[:, int(bias):].astype(np.float64) ** 2).sum(axis=1)
    with np.errstate(divide="ignore"):
        return np.where(S > 0, 1.0 / np.sqrt(S), 0.0)


def cos_bound(dot_b, sq, si, cos):
    """B_cos(q, j) = B'(q, j) sq si + 6 * 2^-24 |cos(q, j)|.  The first term bounds the device's sum (B', scaled as the sum is);
    the second allows for two multiplications and two inverse norms, each rounded once to float32 -- four relative errors of at
    most 2^-24 -- with slack.  Derived, not measured."""
    return np.asarray(dot_b) * np.asarray(sq, dtype=np.float64)[:, None] * np.asarray(si, dtype=np.float64)[None, :] + 6.0 * U32 * np.abs(cos)


def similar_ref(scores, self_id, excluded, topn):
    """The topn best rows of one query, best first, equal scores by row id: `scores` of every catalogue row; `self_id`: the row
    that is the query itself (None: it may be returned); `excluded`: further rows left out (any order, duplicates allowed)."""
    out = np.asarray(excluded, dtype=np.int64).reshape(-1)
    if self_id is not None and 0 <= int(self_id) < len(scores):
        out = np.append(out, int(self_id))
    return recommend_ref.recommend_ref(scores, out, topn)
