"""Host-side reference of the grouped top-n (include/wmf_hip.h, wmf_recommend_topn_grouped) and of the capped list on top of it
(WMF.recommend_capped), in plain NumPy.  Nothing here touches a GPU: tests/test_recommend_grouped_cpu.py checks both against brute
force."""
import numpy as np

import recommend_ref as rref
import serving_ref


def grouped_ref(scores, seen, group_of, n_groups, topn, allow=None):
    """The lists of one row, one per group: list g = recommend_ref(scores, seen + {j : group_of[j] != g} + not allowed, topn).
    `allow`: bool [n_items] or None."""
    group_of = np.asarray(group_of, dtype=np.int64)
    seen = np.asarray(seen, dtype=np.int64)
    barred = np.flatnonzero(~np.asarray(allow, dtype=bool)) if allow is not None else seen[:0]
    return [rref.recommend_ref(scores, np.concatenate([seen, np.flatnonzero(group_of != g), barred]), topn) for g in range(n_groups)]


def capped_ref(scores, seen, group_of, n_groups, topn, per_group, allow=None):
    """The topn best eligible items of one row with at most per_group of any group: a greedy walk down the row's full stable order
    (score descending, equal scores by item id) with one counter per group.  Items of no group (outside [0, n_groups)) are skipped."""
    scores = np.asarray(scores)
    group_of = np.asarray(group_of, dtype=np.int64)
    out_of_play = set(int(s) for s in seen)
    taken, out = np.zeros(n_groups, dtype=np.int64), []
    for j in serving_ref.stable_topn(scores, len(scores)):
        g = int(group_of[j])
        if len(out) == topn:
            break
        if not 0 <= g < n_groups or int(j) in out_of_play or (allow is not None and not allow[j]) or taken[g] >= per_group:
            continue
        taken[g] += 1
        out.append(int(j))
    return np.array(out, dtype=np.int64)


def merge_of_shelves(shelves, scores, topn):
    """The formulation WMF.recommend_capped uses: the keys of a row's lists (grouped_ref at min(per_group, topn)) sorted by (score
    descending, item ascending), the first topn taken."""
    ids = np.concatenate([np.asarray(s, dtype=np.int64) for s in shelves]) if len(shelves) else np.zeros(0, dtype=np.int64)
    return np.array(sorted(ids, key=lambda j: (-scores[j], j))[:topn], dtype=np.int64)


def scan_lds_bytes(tps, ld, n_waves, n_groups):
    """The dynamic LDS of a grouped scan (recmodel_amd/csrc: wmf_scan_stage_bytes + rec_grouped_lds_bytes): two stages of tps x 16
    item rows ((ld / 4) | 1 pieces of 16 bytes apart), per wave 16 x n_groups thresholds (8 B) and counts (4 B) and a 256-bin
    histogram."""
    return 2 * tps * 16 * ((ld >> 2) | 1) * 16 + n_waves * 16 * n_groups * 12 + n_waves * 256 * 4


WIDTH_CLASSES = ((4, 64), (2, 144), (1, 272))                       # (tiles per stage, the widest ld of the class)
