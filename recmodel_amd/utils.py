"""Helpers around a trained model; same call surface as RecModel/utils.py."""
import numpy as np
import scipy.sparse

COVERAGE_BATCH_USERS = 8192       # users per recommend() call of test_coverage


def test_coverage(cls, Train, topN):
    """How often each item is among a user's ``topN`` recommendations, over all users of ``Train``; items the user has an
    entry for in ``Train`` are never recommended.  RecModel/utils.py:3-17.

    A model with ``recommend`` (WMF) answers a whole batch of users per call on the device; any other model is asked user by
    user through ``rank``, as the reference does.

    Deviation from the reference: it allocates ``Train.shape[0]`` counters -- the number of USERS -- and indexes them with
    item ids, which raises IndexError as soon as an item id >= n_users is recommended.  Here there is one int32 counter per
    item, ``Train.shape[1]`` of them."""
    Train = scipy.sparse.csr_matrix(Train)
    n_users, n_items = Train.shape
    counts = np.zeros(n_items, dtype=np.int64)
    if hasattr(cls, "recommend"):
        for u0 in range(0, n_users, COVERAGE_BATCH_USERS):
            got = np.asarray(cls.recommend(np.arange(u0, min(u0 + COVERAGE_BATCH_USERS, n_users)), topn=topN, exclude=Train))
            got = got[got >= 0]
            counts += np.bincount(got, minlength=n_items)
    else:
        everything = np.arange(n_items, dtype=np.int32)
        for user in range(n_users):
            unseen = np.delete(everything, Train.indices[Train.indptr[user]:Train.indptr[user + 1]])
            best = np.asarray(cls.rank(users=user, items=unseen, topn=topN)).reshape(-1)[:topN]
            counts += np.bincount(best, minlength=n_items)
    return counts.astype(np.int32)


test_coverage.__test__ = False    # (a library function, not a test: pytest must not collect it)
