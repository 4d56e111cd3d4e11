"""The ids every serving call of WMF takes -- predict, rank (one user and a list), recommend, similar_items, similar_users -- go
through one check: an id outside [-n, n) of its side is an IndexError with the call's own message, raised before the GPU is asked
for; an id inside, -n and n - 1 included, gets past it (and negative ids count from the end, which the GPU model tests see)."""
import numpy as np
import pytest

N_USERS, N_ITEMS, DIM = 5, 12, 3
# name: (the call on (model, user ids, item ids), the sides whose ids it takes, its message)
CALLS = {
    "predict": (lambda m, u, i: m.predict(u, i), ("users", "items"), "user or item index out of bounds"),
    "rank-one-user": (lambda m, u, i: m.rank(i, u[0], 2), ("users", "items"), "user or item index out of bounds"),
    "rank-user-list": (lambda m, u, i: m.rank(i, u, 2), ("users", "items"), "user or item index out of bounds"),
    "recommend": (lambda m, u, i: m.recommend(u, topn=2), ("users",), "user index out of bounds"),
    "similar_items": (lambda m, u, i: m.similar_items(i, topn=2), ("items",), "item index out of bounds"),
    "similar_users": (lambda m, u, i: m.similar_users(u, topn=2), ("users",), "user index out of bounds"),
}


def _model():
    from recmodel_amd import WMF
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=DIM, gamma=0.1, weighted=True)
    m.users = (np.arange(N_USERS * DIM, dtype=np.float32).reshape(N_USERS, DIM) - 7) / 4
    m.items = (np.arange(N_ITEMS * DIM, dtype=np.float32).reshape(N_ITEMS, DIM) - 17) / 8
    return m


@pytest.mark.parametrize("name", list(CALLS))
def test_ids_are_checked_against_both_bounds_before_the_gpu(name):
    import torch
    from recmodel_amd import _lib
    call, sides, message = CALLS[name]
    m = _model()
    n = {"users": N_USERS, "items": N_ITEMS}
    inside = {side: [-n[side], n[side] - 1] for side in n}
    for side in sides:
        for bad in (n[side], -n[side] - 1):
            ids = dict(inside, **{side: [bad, 0]})
            with pytest.raises(IndexError) as err:
                call(m, ids["users"], ids["items"])
            assert str(err.value) == message, (name, side, bad)
    if not torch.cuda.is_available():                               # past the check: the next thing the call wants is the GPU
        with pytest.raises(_lib.WmfLibraryError):
            call(m, inside["users"], inside["items"])
