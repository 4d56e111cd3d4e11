"""Host-side reference of the full-catalogue top-n with exclusions (include/wmf_hip.h, wmf_recommend_topn), in plain NumPy.
Nothing here touches a GPU: tests/test_recommend_cpu.py checks it against the CPU reference implementation's rank()."""
import numpy as np

import serving_ref


def recommend_ref(scores, seen, topn):
    """The topn best eligible items of one user, best first, equal scores by item id.  `scores`: the user's score of every
    item of the catalogue (int64 or float64); `seen`: item ids left out (any order, duplicates allowed)."""
    scores = np.asarray(scores)
    elig = np.setdiff1d(np.arange(len(scores)), seen)
    return elig[serving_ref.stable_topn(scores[elig], min(topn, len(elig)))]


def padded_rows(rows, topn, fill, dtype):
    """[len(rows), topn]: every row's entries, then `fill`."""
    out = np.full((len(rows), topn), fill, dtype=dtype)
    for b, row in enumerate(rows):
        out[b, :len(row)] = row
    return out


def csr_of(rows):
    """(indptr int64, indices int32 with one spare element) of a list of id lists, stored as given."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(1, dtype=np.int64)]).astype(np.int32)
    return indptr, indices
