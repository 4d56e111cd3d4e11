"""Host-side reference of the exact full-catalogue ranks (include/wmf_hip.h, wmf_rank_positions) and of the metrics
RecModel.eval_ranking derives from them, in plain NumPy.  Nothing here touches a GPU: tests/test_rankpos_cpu.py checks it against
tests/recommend_ref.py and against hand-computed numbers."""
import numpy as np

SEEN, BEYOND = -1, -2                                             # WMF_RANKPOS_SEEN, WMF_RANKPOS_BEYOND


def rank_positions_ref(scores, seen, targets):
    """For every target the number of eligible items -- ids of range(len(scores)) not in `seen` -- that stand strictly above it
    in the order (score descending, id ascending); SEEN for a target that is in `seen`.  `scores`: one user's score of every
    item (int64 or float64); `seen`, `targets`: item ids in any order, duplicates allowed.  int64[len(targets)]."""
    scores = np.asarray(scores)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    eligible = np.ones(len(scores), dtype=bool)
    eligible[np.asarray(seen, dtype=np.int64).reshape(-1)] = False
    ids = np.arange(len(scores))
    out = np.empty(len(targets), dtype=np.int64)
    for p, t in enumerate(targets):
        above = (scores > scores[t]) | ((scores == scores[t]) & (ids < t))
        out[p] = (above & eligible).sum() if eligible[t] else SEEN
    return out


def ranking_metrics_ref(ranks_per_user, topn):
    """{"Recall@k", "Precision@k", "ARHR@k", "NDCG@k" for k in topn} from one array of ranks per user (SEEN = a miss that stays
    in the denominators).  n_test = all targets, U = users with at least one target:
      Recall@k = hits_k / n_test,  Precision@k = hits_k / (k U),  ARHR@k = sum_{rank < k} 1 / (rank + 1) / n_test,
      NDCG@k = mean over the U users of sum_{rank < k} 1 / log2(rank + 2) / sum_{i < min(k, T_u)} 1 / log2(i + 2),
    T_u = the user's distinct targets that are not seen (distinct unseen items have distinct ranks); ideal 0 contributes 0."""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in ranks_per_user]
    rows = [r for r in rows if len(r)]
    n_test, n_users = sum(len(r) for r in rows), len(rows)
    out = {}
    for k in (int(k) for k in topn):
        hits = arhr = ndcg = 0.0
        for r in rows:
            hit = r[(r >= 0) & (r < k)]
            hits += len(hit)
            arhr += sum(1.0 / (x + 1.0) for x in hit)
            ideal = sum(1.0 / np.log2(i + 2.0) for i in range(min(k, len(set(r[r >= 0].tolist())))))
            if ideal > 0:
                ndcg += sum(1.0 / np.log2(x + 2.0) for x in hit) / ideal
        out[f"Recall@{k}"] = hits / n_test if n_test else float("nan")
        out[f"Precision@{k}"] = hits / (k * n_users) if n_users else float("nan")
        out[f"ARHR@{k}"] = arhr / n_test if n_test else float("nan")
        out[f"NDCG@{k}"] = ndcg / n_users if n_users else float("nan")
    return out
