"""WMF.explain on small trained models (k = 16, 64 + bias, 128 + bias, and a float64 model served from its float32 copies) against
tests/explain_ref.py and the oracle's fold-in: the totals are predict on recompute_factors[_bias](items, C_u, gamma); the top-k
lists are the reference's up to entries whose reference contributions lie within the gate of each other; the shapes of the
public surface (topk=None, an int user, more targets than one device call takes, small batches, -1 slots) and the cache rule of
the device copies."""
import numpy as np
import pytest
import scipy.sparse as sp

import explain_ref as ref
from conftest import record_error
from oracle import wmf_oracle as orc

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 600
GAMMA = 0.1
MODELS = {"k16": (16, False, 1), "k64-bias": (64, True, 1), "k128-bias": (128, True, 1), "k16-f64": (16, False, 2)}
USERS = np.array([0, 1, 2, 3, 17, 17, 101, 250, N_USERS - 1, -2])


@pytest.fixture(scope="module")
def train_mat():
    from recmodel_amd import synth
    indptr, indices, counts = synth.make_counts(N_USERS, N_ITEMS, 9, seed=5)
    return synth.to_scipy(indptr, indices, counts, (N_USERS, N_ITEMS)).astype(np.float64)


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, train_mat):
    from recmodel_amd import WMF
    dim, bias, cores = MODELS[request.param]
    m = WMF(num_items=N_ITEMS, num_users=N_USERS, dim=dim, gamma=GAMMA, weighted=True, bias=bias)
    m.train(utility_mat=train_mat, iterations=2, eval_mat=train_mat, count_mat=train_mat, cores=cores)
    assert m.items.dtype == (np.float64 if cores > 1 else np.float32) and not m.items.flags.writeable
    m.case_name = request.param
    return m


def _reference(model, train_mat, users, targets):
    """The rows ``users`` of the count matrix as the device reads them (float32 factors, float32 confidences) through ref64 and
    restated32, and the oracle's fold-in scores in float64 and float32.  Returns a dict."""
    bias = int(model.bias is True)
    Y32 = model.items.astype(np.float32)
    u = np.where(users < 0, users + N_USERS, users)
    rows = train_mat[u]
    conf = (10 * np.log1p(rows.data.astype(np.float32).astype(np.float64))).astype(np.float32)
    indptr, indices = rows.indptr.astype(np.int64), rows.indices.astype(np.int32)
    targets = np.asarray(targets, dtype=np.int32)
    W32 = ref.whitening(Y32, bias, GAMMA).astype(np.float32)
    c64, t64 = ref.ref64(Y32, bias, GAMMA, indptr, indices, conf, targets)
    c32, t32 = ref.restated32(Y32, bias, W32, indptr, indices, conf, targets)
    C = sp.csr_matrix((conf, indices, indptr), shape=(len(u), N_ITEMS))
    step = orc.recompute_factors_bias if bias else orc.recompute_factors
    fold = {}
    for dt in ("float64", "float32"):
        X = step(Y32.astype(dt), C.astype(dt), GAMMA, dtype=dt)
        fold[dt] = np.stack([orc.predict(X, Y32.astype(dt), np.full(targets.shape[1], k), np.maximum(targets[k], 0), bias=bool(bias))
                             for k in range(len(u))]).astype(np.float64)
        fold[dt][targets < 0] = 0
    gate = ref.GATE_MARGIN * ref.pair_errors(c32, c64, indptr) + ref.GATE_FLOOR
    return dict(indptr=indptr, indices=indices, c64=c64, t64=t64, t32=t32.astype(np.float64), fold64=fold["float64"],
                fold32=fold["float32"], gate=gate, targets=targets)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_explain_recommendations(model, train_mat):
    """explain(u, recommend(u, 5, exclude=Train), Train): the totals are the fold-in scores, the lists are the reference's."""
    rec = model.recommend(USERS, 5, exclude=train_mat)
    assert rec.shape == (len(USERS), 5) and (rec >= 0).all()
    total, hist, best = model.explain(USERS, rec, train_mat, topk=4)
    assert total.dtype == np.float32 and total.shape == (len(USERS), 5)
    assert hist.dtype == np.int64 and hist.shape == (len(USERS), 5, 4) and best.dtype == np.float32 and best.shape == hist.shape
    r = _reference(model, train_mat, USERS, rec)
    assert np.abs(r["t64"] - r["fold64"]).max() <= 1e-9 * max(1.0, np.abs(r["fold64"]).max())      # the identity, in float64
    # the fold-in tolerance: the two float32 paths' own errors against float64 (the restatement's totals, the oracle's float32
    # fold-in), per row the worst of its targets, with the margin of 4 and the floor of 8 ulps of the row's largest score
    e1 = np.abs(r["t32"] - r["t64"]).max(axis=1)
    e2 = np.abs(r["fold32"] - r["fold64"]).max(axis=1)
    tol = ref.GATE_MARGIN * (e1 + e2) + ref.GATE_FLOOR * np.abs(r["fold64"]).max(axis=1)
    err = np.abs(total - r["fold32"]).max(axis=1)
    print(f"{model.case_name}: fold-in |device - oracle32| {err.max():.3e}, restated {e1.max():.3e}, oracle32 {e2.max():.3e}, "
          f"worst err / tol {np.max(err / tol):.3f}, |device - float64| {np.abs(total - r['fold64']).max():.3e}")
    record_error("explain_model", **{model.case_name + "_foldin_device_vs_oracle32": err.max(), model.case_name + "_restated_total": e1.max(),
                                     model.case_name + "_oracle32_total": e2.max(),
                                     model.case_name + "_device_vs_float64": np.abs(total - r["fold64"]).max()})
    assert (err <= tol).all(), (err, tol)
    # the lists: position p holds an entry whose reference contribution is within the pair's gate of the p-th largest
    worst = 0.0
    for b in range(len(USERS)):
        lo, hi = int(r["indptr"][b]), int(r["indptr"][b + 1])
        keep = min(4, hi - lo)
        items = r["indices"][lo:hi]
        for t in range(5):
            c = r["c64"][lo:hi, t]
            scale = max(np.abs(c).max(initial=0), ref.TINY)
            gate = r["gate"][b, t] * scale
            order = np.argsort(-c, kind="stable")[:keep]
            assert (hist[b, t, keep:] == -1).all() and (best[b, t, keep:] == 0).all()
            got = hist[b, t, :keep]
            assert len(np.unique(got)) == keep and np.isin(got, items).all()
            pos = np.array([int(np.nonzero(items == g)[0][0]) for g in got], dtype=np.int64)
            assert (np.diff(best[b, t, :keep]) <= 0).all()
            assert (np.abs(c[pos] - c[order]) <= gate).all(), (b, t, c[pos], c[order], gate)
            assert (np.abs(best[b, t, :keep] - c[pos]) <= gate).all(), (b, t)
            if keep:
                worst = max(worst, float(np.abs(best[b, t, :keep] - c[pos]).max() / gate))
    print(f"{model.case_name}: listed contributions, worst error / gate {worst:.3f}")
    record_error("explain_model", **{model.case_name + "_listed_worst_over_gate": worst})
    assert np.array_equal(_bits(total[4]), _bits(total[5]))          # the same user twice


def test_shapes_of_the_public_surface(model, train_mat):
    items = np.array([[0, 5, -1, N_ITEMS - 1, 7, 5]] * len(USERS))
    items[:, 1] = [train_mat[u].indices[0] for u in np.where(USERS < 0, USERS + N_USERS, USERS)]     # an item of the user's own history
    items[:, 5] = items[:, 1]                                        # the same item twice
    total, hist, best = model.explain(USERS, items, train_mat, topk=3)
    full = model.explain(USERS, items, train_mat, topk=None)
    assert len(full) == 4 and np.array_equal(_bits(full[0]), _bits(total))
    _, indptr, indices, contrib = full
    rows = train_mat[np.where(USERS < 0, USERS + N_USERS, USERS)]
    assert np.array_equal(indptr, rows.indptr) and np.array_equal(indices, rows.indices) and indices.dtype == np.int64
    assert contrib.shape == (rows.nnz, items.shape[1]) and contrib.dtype == np.float32
    assert (contrib[:, 2] == 0).all() and (total[:, 2] == 0).all() and (hist[:, 2] == -1).all() and (best[:, 2] == 0).all()      # the -1 slot
    assert np.array_equal(_bits(contrib[:, 1]), _bits(contrib[:, 5])) and np.array_equal(_bits(total[:, 1]), _bits(total[:, 5]))
    for b in range(len(USERS)):
        lo, hi = indptr[b], indptr[b + 1]
        keep = min(3, hi - lo)
        for t in (0, 1, 3, 4, 5):
            order = np.argsort(-contrib[lo:hi, t], kind="stable")[:keep]
            assert np.array_equal(hist[b, t, :keep], indices[lo:hi][order]) and (hist[b, t, keep:] == -1).all()
            assert np.array_equal(_bits(best[b, t, :keep]), _bits(contrib[lo:hi, t][order])) and (best[b, t, keep:] == 0).all()
    # an int user (negative ids count from the end) drops the first axis; 1-D items for several users drop the target axis
    one = model.explain(-2, items[-1], train_mat, topk=3)
    assert one[0].shape == (6,) and one[1].shape == (6, 3) and all(np.array_equal(a, b[-1]) for a, b in zip(one, (total, hist, best)))
    assert np.array_equal(_bits(model.explain(int(USERS[3]), items[3], train_mat, topk=None)[0]), _bits(total[3]))
    flat = model.explain(USERS, items[:, 1], train_mat, topk=3)
    assert flat[0].shape == (len(USERS),) and flat[1].shape == (len(USERS), 3)
    assert np.array_equal(_bits(flat[0]), _bits(total[:, 1])) and np.array_equal(flat[1], hist[:, 1]) and np.array_equal(_bits(flat[2]), _bits(best[:, 1]))
    # defaults: topk = 10, the transform of train
    assert model.explain(USERS, items, train_mat)[1].shape == (len(USERS), 6, 10)
    other = model.explain(USERS, items, train_mat, topk=None, pre_process_count="linear", alpha=2)
    assert not np.array_equal(other[3], contrib)
    assert model.explain([], np.zeros((0, 3), dtype=np.int64), train_mat)[0].shape == (0, 3)


def test_more_targets_than_one_call_and_small_batches(model, train_mat, monkeypatch):
    from recmodel_amd import wmf_model
    assert wmf_model.EXPLAIN_MAX_TARGETS == ref.MAX_TARGETS
    rng = np.random.default_rng(8)
    users = np.arange(0, N_USERS, 3)
    items = rng.integers(0, N_ITEMS, (len(users), 2 * ref.MAX_TARGETS + 5))
    total, indptr, indices, contrib = model.explain(users, items, train_mat, topk=None)
    assert total.shape == items.shape and contrib.shape == (indptr[-1], items.shape[1])
    for t0 in (0, ref.MAX_TARGETS, 2 * ref.MAX_TARGETS):
        part = model.explain(users, items[:, t0:t0 + ref.MAX_TARGETS], train_mat, topk=None)
        assert np.array_equal(_bits(part[0]), _bits(total[:, t0:t0 + ref.MAX_TARGETS]))
        assert np.array_equal(_bits(part[3]), _bits(contrib[:, t0:t0 + ref.MAX_TARGETS]))
    monkeypatch.setattr(wmf_model, "RECOMMEND_BATCH_USERS", 48)
    again = model.explain(users, items, train_mat, topk=None)
    assert np.array_equal(_bits(again[0]), _bits(total)) and np.array_equal(_bits(again[3]), _bits(contrib))


def test_explain_follows_the_public_arrays(model, train_mat):
    """The cache rule of _device_factors: the whitening of a trained model's frozen items is computed once (per gamma); a writable
    array is uploaded, and whitened, again on every call, so an in-place edit shows."""
    trained = model.items
    try:
        u = 7
        hist_item = int(train_mat[u].indices[0])
        items = np.array([hist_item, 3, 11])
        before = model.explain(u, items, train_mat, topk=None)
        W = model._white[float(model.gamma)]
        again = model.explain(u, items, train_mat, topk=None)
        assert model._white[float(model.gamma)] is W and np.array_equal(_bits(again[3]), _bits(before[3]))     # frozen: by identity
        gamma = model.gamma
        model.gamma = 2 * gamma                                      # another regulariser: another whitening, both kept
        assert not np.array_equal(model.explain(u, items, train_mat, topk=None)[3], before[3]) and len(model._white) == 2
        model.gamma = gamma
        assert model._white[float(gamma)] is W
        model.items = trained.copy()                                 # writable, the same values
        same = model.explain(u, items, train_mat, topk=None)
        assert np.array_equal(_bits(same[3]), _bits(before[3])) and model._white[float(gamma)] is not W
        model.items[hist_item] *= 0.5                                # in place: the edit shows in the next call
        edited = model.explain(u, items, train_mat, topk=None)
        assert not np.array_equal(edited[3], before[3])
    finally:
        model.items = trained
    assert np.array_equal(_bits(model.explain(u, items, train_mat, topk=None)[3]), _bits(before[3]))
