"""``RecModel`` base class: the evaluation surface every model shares.

Host-side mirror of RecModel/base_model.py:34-179 for the WMF path.  ``eval_prec`` (the call
``WMF.train`` makes every iteration, wmf_model.py:163) is answered by the model's device kernel
through ``_eval_sums``; ``eval_topn`` / ``compute_hit`` keep the reference's NumPy RNG call
sequence so a seeded run samples the same negatives.
"""
from functools import partial
from multiprocessing import Pool

import numpy as np
import scipy.sparse

RANKPOS_SEEN = -1                 # WMF_RANKPOS_SEEN of include/wmf_hip.h: the target is in the user's seen list, never recommended


def iter_rows_two_matrices(A, B):
    """Per row: (row, A data, A indices, B data, B indices).  base_model.py:10-20."""
    for row in range(A.shape[0]):
        a0, a1 = A.indptr[row], A.indptr[row + 1]
        b0, b1 = B.indptr[row], B.indptr[row + 1]
        yield row, A.data[a0:a1], A.indices[a0:a1], B.data[b0:b1], B.indices[b0:b1]


def iter_rows_mat(A):
    """Per row: (row, data, indices).  base_model.py:23-31."""
    for row in range(A.shape[0]):
        a0, a1 = A.indptr[row], A.indptr[row + 1]
        yield row, A.data[a0:a1], A.indices[a0:a1]


def ranking_inputs(test_mat, exclude, users, shape=None):
    """The arguments of ``rank_positions`` / ``eval_ranking`` checked and canonicalised on copies: (users int64 with negative
    indices resolved, test_mat[users], exclude[users] or None), both CSR with duplicates summed and indices sorted; every
    stored entry counts, stored zeros too.  ``users`` None: the rows of ``test_mat`` with stored entries.  ValueError for
    a matrix that is not sparse or not of ``shape`` (default: the shape of ``test_mat``), IndexError for a user out of bounds."""
    if not scipy.sparse.issparse(test_mat) or (shape is not None and test_mat.shape != tuple(shape)):
        raise ValueError(f"test_mat must be a sparse matrix of shape {shape}, got {getattr(test_mat, 'shape', None)}")
    shape = tuple(test_mat.shape)
    if exclude is not None and (not scipy.sparse.issparse(exclude) or exclude.shape != shape):
        raise ValueError(f"exclude must be a sparse matrix of shape {shape}, got {getattr(exclude, 'shape', None)}")
    u = None
    if users is not None:
        u = np.atleast_1d(np.asarray(users)).reshape(-1).astype(np.int64)
        if len(u) and (u.min() < -shape[0] or u.max() >= shape[0]):
            raise IndexError("user index out of bounds")
        u = np.where(u < 0, u + shape[0], u)

    def canonical(mat):
        mat = scipy.sparse.csr_matrix(mat, copy=True)
        mat.sum_duplicates()
        mat.sort_indices()
        return mat
    test = canonical(test_mat)
    if u is None:
        u = np.flatnonzero(np.diff(test.indptr)).astype(np.int64)
    return u, test[u], (canonical(exclude)[u] if exclude is not None else None)              # (row selection keeps a row's order)


def ranking_metrics(indptr, ranks, topn):
    """Recall / Precision / ARHR / NDCG at every k of ``topn`` from exact ranks: ``ranks[indptr[j]:indptr[j + 1]]`` are the
    0-based places of user j's targets among the unseen items of the whole catalogue, RANKPOS_SEEN for a target the user has
    seen (a miss that stays in the denominators).  float64 on the host.  n_test = targets, U = users with at least one:
    Recall@k = hits_k / n_test (the reference's micro convention, base_model.py:143), Precision@k = hits_k / (k U),
    ARHR@k = sum over hits of 1 / (rank + 1) / n_test, NDCG@k = the mean over the U users of sum over hits of
    1 / log2(rank + 2) divided by the ideal sum_{i < min(k, T_u)} 1 / log2(i + 2), T_u the user's distinct unseen targets (a
    user whose ideal is 0 contributes 0)."""
    indptr, ranks = np.asarray(indptr, dtype=np.int64), np.asarray(ranks, dtype=np.int64)
    per_user = np.diff(indptr)
    n_test, n_u = int(per_user.sum()), int((per_user > 0).sum())
    out = {}
    for k in (int(k) for k in topn):
        hit = (ranks >= 0) & (ranks < k)
        hits = float(hit.sum())
        gain = np.where(hit, 1.0 / np.log2(np.where(hit, ranks, 0) + 2.0), 0.0)
        ndcg = 0.0
        for j in np.flatnonzero(per_user):
            row = slice(indptr[j], indptr[j + 1])
            distinct = len(np.unique(ranks[row][ranks[row] >= 0]))          # distinct unseen items have distinct ranks
            ideal = float((1.0 / np.log2(np.arange(min(k, distinct)) + 2.0)).sum())
            if ideal > 0:
                ndcg += float(gain[row].sum()) / ideal
        out[f"Recall@{k}"] = hits / n_test if n_test else float("nan")
        out[f"Precision@{k}"] = hits / (k * n_u) if n_u else float("nan")
        out[f"ARHR@{k}"] = float(np.where(hit, 1.0 / (np.where(hit, ranks, 0) + 1.0), 0.0).sum()) / n_test if n_test else float("nan")
        out[f"NDCG@{k}"] = ndcg / n_u if n_u else float("nan")
    return out


class RecModel:
    """Common evaluation scheme; subclasses implement train / predict / rank (base_model.py:34-49)."""

    def train(self):
        pass

    def predict(self, user_item):
        pass

    def rank(self, items, user, topn=None):
        pass

    # -------------------------------------------------------------- accuracy metrics
    def _eval_sums(self, utility_mat):
        """(sum sq err, sum abs err, count) over stored non-zero entries; subclasses provide it."""
        raise NotImplementedError

    def eval_prec(self, utility_mat, metric='mse'):
        """MSE / RMSE / MAE of predict() on the non-zero entries.  base_model.py:150-179."""
        metric = metric.upper()
        if metric not in ('MSE', 'RMSE', 'MAE'):
            raise ValueError("Metric {metric} is not implemented.")
        sq, ab, cnt = self._eval_sums(utility_mat)
        if cnt == 0:
            return float('nan')          # np.mean of an empty selection
        if metric == 'RMSE':
            return np.sqrt(sq / cnt)
        if metric == 'MSE':
            return sq / cnt
        return ab / cnt

    # -------------------------------------------------------------- sampled Recall@N
    def compute_hit(self, elem, rand_sampled, topn, dtype="float32"):
        """Hits of one user's test items among ``rand_sampled`` random candidates.
        base_model.py:51-98 (same np.random call order: candidates, then the slot)."""
        user, _, _, test_dat, test_idx = elem
        if len(test_dat) == 0:
            return np.zeros(topn.shape, dtype=dtype)
        candidates = np.random.randint(0, self.num_items, size=(rand_sampled + 1))
        slot = np.random.randint(0, rand_sampled - (2 * topn.max()))
        hits = np.zeros(topn.shape, dtype=dtype)
        for item in test_idx:
            candidates[slot] = item
            best = self.rank(items=candidates, users=user, topn=topn.max())
            for pos in range(len(topn)):
                if item in best[:topn[pos]]:
                    hits[pos] += 1
        return hits

    def _hit_counts(self, pair_user, pair_item, pair_row, candidates, slot, topn):
        """Hook for a device implementation of compute_hit over all test entries at once: entry p is
        (pair_user[p], pair_item[p]) with candidate row ``candidates[pair_row[p]]`` whose position
        ``slot[pair_row[p]]`` holds the test item.  Returns hits per topn, or None when not provided."""
        return None

    def eval_topn(self, test_mat, train_mat=None, eval_mat=None, topn=[10], rand_sampled=1000, cores=1,
                  random_state=None, dtype='float32'):
        """Recall@N with sampled negatives.  base_model.py:100-148.

        The random candidates are drawn on the host exactly as compute_hit draws them (users in row order,
        only users with test entries; candidates first, then the slot), so a seeded call samples what the
        reference samples.  Models that provide ``_hit_counts`` then rank every test entry in one device
        launch (``cores`` has no meaning there); others go through ``rank`` entry by entry like the reference."""
        super_mat = test_mat
        if train_mat is not None:
            super_mat += train_mat
        if eval_mat is not None:
            super_mat += eval_mat
        if random_state is not None:
            np.random.seed(random_state)
        if not isinstance(topn, np.ndarray):
            raise ValueError("Topn has to be a np.array")
        n_test = len(test_mat.nonzero()[0])
        if type(self)._hit_counts is RecModel._hit_counts:
            hits = np.zeros(topn.shape, dtype=dtype)
            if cores == 1:
                for elem in iter_rows_two_matrices(super_mat, test_mat):
                    hits += self.compute_hit(elem, rand_sampled=rand_sampled, topn=topn)
            else:
                with Pool(cores) as pool:
                    fn = partial(self.compute_hit, rand_sampled=rand_sampled, topn=topn)
                    hits = np.stack(pool.map(fn, iter_rows_two_matrices(super_mat, test_mat))).sum(axis=0)
        else:
            per_row = np.diff(test_mat.indptr)
            rows = np.flatnonzero(per_row)
            cand = np.empty((len(rows), rand_sampled + 1), dtype=np.int32)
            slot = np.empty(len(rows), dtype=np.int32)
            for k in range(len(rows)):                            # the draws of compute_hit, in its order
                cand[k] = np.random.randint(0, self.num_items, size=(rand_sampled + 1))
                slot[k] = np.random.randint(0, rand_sampled - (2 * topn.max()))
            pair_user = np.repeat(np.arange(test_mat.shape[0]), per_row)
            pair_row = np.repeat(np.arange(len(rows)), per_row[rows])
            hits = np.asarray(self._hit_counts(pair_user, test_mat.indices, pair_row, cand, slot, topn)).astype(dtype)
        recall = hits / n_test
        return {f"Recall@{topn[pos]}": recall[pos] for pos in range(len(topn))}

    # -------------------------------------------------------------- exact full-catalogue ranking metrics
    def _rank_positions(self, test_mat, exclude, users):
        """Hook for a device implementation of the exact ranks: ``(indptr, indices, ranks)`` as ``WMF.rank_positions``
        returns them, or None when not provided."""
        return None

    def eval_ranking(self, test_mat, train_mat=None, topn=np.array([10]), users=None):
        """Unsampled Recall@k, Precision@k, ARHR@k and NDCG@k over the whole catalogue: every stored entry of ``test_mat``
        (stored zeros too) is a held-out item whose exact place among the items the user has no entry for in ``train_mat`` is
        counted -- no sampled negatives, unlike ``eval_topn``, and the seen items are left out.  ``users``: the rows to
        evaluate (default: those with test entries).  A held-out item that is also in ``train_mat`` is a miss.  Returns
        ``{"Recall@10": ..., "Precision@10": ..., "ARHR@10": ..., "NDCG@10": ...}`` for every k of ``topn`` (see
        ``ranking_metrics``).  Neither matrix is modified.

        A model that provides ``_rank_positions`` counts on the device; any other is asked user by user through
        ``rank(items=unseen, users=u, topn=None)`` and the targets are looked up in the returned order."""
        if not isinstance(topn, np.ndarray):
            raise ValueError("Topn has to be a np.array")
        if type(self)._rank_positions is not RecModel._rank_positions:
            indptr, _, ranks = self._rank_positions(test_mat, train_mat, users)
            return ranking_metrics(indptr, ranks, topn)
        u, test, seen = ranking_inputs(test_mat, train_mat, users)
        everything = np.arange(test.shape[1], dtype=np.int32)
        ranks = np.empty(test.nnz, dtype=np.int64)
        for j, user in enumerate(u):
            row = slice(test.indptr[j], test.indptr[j + 1])
            if row.start == row.stop:
                continue
            unseen = everything if seen is None else np.delete(everything, seen.indices[seen.indptr[j]:seen.indptr[j + 1]])
            place = np.full(test.shape[1], RANKPOS_SEEN, dtype=np.int64)
            if len(unseen):
                order = np.asarray(self.rank(items=unseen, users=int(user), topn=None))
                place[order] = np.arange(len(order))
            ranks[row] = place[test.indices[row]]
        return ranking_metrics(test.indptr, ranks, topn)
