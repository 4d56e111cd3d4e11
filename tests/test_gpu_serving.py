"""The kernels behind the numbers a user reads -- predict, rank, the MSE of early stopping, Recall@N -- one entry point at a time
through the C ABI, per element, at every width class (csrc/wmf_eval.hip, csrc/wmf_rank.hip, the tail of csrc/wmf_solve.hip).

wmf_pair_score (csrc/wmf_common.h) walks a row in 16-byte pieces, 16 lanes wide: one trip up to f = 64, five at f = 260; the MFMA tile
kernel of the batched rank pads the piece count to a multiple of 4.  WIDTHS has every trip count, every piece count modulo 4
and every bench width, each with and without the bias column, a handful also with a wider leading dimension.

Two input classes (tests/serving_ref.py): EXACT -- integers in -3 .. 3, so the device must equal the int64 host result bit for
bit, ties are real ties and any dropped, doubled or mis-indexed column moves a score by at least 1 -- and ROUNDED -- standard
normal float32 against float64 on the same numbers, every score within the derived bound B(u, i) = 2 (f + 2) 2^-24 (sum of
the absolute terms); the measured worst err / B goes to record_error (profiles/r06_parity_errors.json, keys serving_*).  Each grid-stride
loop is run past its cap once, at a small width.  No case passes an undersized buffer: "empty" cases use valid one-element
arrays and check that nothing was written."""
import functools

import numpy as np
import pytest
import torch

import serving_ref as ref
from conftest import record_error

pytestmark = pytest.mark.gpu

WIDTHS = (1, 4, 5, 16, 63, 64, 65, 100, 128, 129, 144, 192, 193, 256, 257, 260)
# these also at a wider leading dimension: ld + 4, 100 at 108 (with 5 at 12 the piece counts that are 3 modulo 4, which no width
# of the list has at its own ld), 260 at 272, the largest
LD_EXTRA = {5: 4, 64: 4, 100: 8, 129: 4, 257: 4, 260: 12}
CASES = [(f, b, 0) for f in WIDTHS for b in (0, 1) if f >= 2 or not b] + [(f, b, e) for f, e in LD_EXTRA.items() for b in (0, 1)]
_PIECES = {((f + 3) // 4 * 4 + e) // 4 for f, _, e in CASES}      # 16-byte pieces per row
assert {n % 4 for n in _PIECES} == {0, 1, 2, 3} and {(n + 15) // 16 for n in _PIECES} == {1, 2, 3, 4, 5} and max(_PIECES) == 68
N_USERS, N_ITEMS = 40, 300
SENTINEL = -12345.0
case = pytest.mark.parametrize("f,bias,extra", CASES, ids=[f"f{f}-b{b}" + (f"-ld+{e}" if e else "") for f, b, e in CASES])


# ------------------------------------------------------------------------------------------------------------------ helpers
def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _ld(f, extra=0):
    ld = _api()[1].wmf_ld_for(f) + extra
    assert ld % 4 == 0 and f <= ld <= 272
    return ld


@functools.lru_cache(maxsize=None)
def _host(f, cls, n_users=N_USERS, n_items=N_ITEMS):
    make = ref.exact_factors if cls == "exact" else ref.rounded_factors
    Uf, If = make(n_users, f, 10 * f + 1), make(n_items, f, 10 * f + 2)
    Uf.setflags(write=False)
    If.setflags(write=False)
    return Uf, If


@functools.lru_cache(maxsize=64)
def _device(f, ld, cls, n_users=N_USERS, n_items=N_ITEMS):
    Uf, If = _host(f, cls, n_users, n_items)
    return _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld))


@functools.lru_cache(maxsize=None)
def _matrix(f, bias):
    """int64 scores of every (user, item) of the EXACT class at this width: computed once, shared, never written."""
    Uf, If = _host(f, "exact")
    M = ref.score_matrix_int(Uf, If, np.arange(N_USERS), np.arange(N_ITEMS), bias)
    M.setflags(write=False)
    return M


def _record(kernel, f, bias, ld, ratio):
    record_error(f"serving_{kernel}", **{f"f{f}_bias{bias}_ld{ld}": ratio})


def _predict(Ud, Id, f, ld, bias, ui, ii):
    _lib, lib, _ptr, _stream = _api()
    n = max(len(ui), len(ii))
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ui_d, ii_d = _dev(ui, np.int32), _dev(ii, np.int32)            # named: a temporary's memory is handed out again at once
    _lib.check(lib.wmf_predict_pairs(_ptr(Ud), _ptr(Id), f, ld, bias, _ptr(ui_d), len(ui), _ptr(ii_d), len(ii), _ptr(out), _stream()))
    return out.cpu().numpy()


def _eval(Ud, Id, f, ld, bias, indptr, indices, values, n):
    _lib, lib, _ptr, _stream = _api()
    ws = torch.empty(int(lib.wmf_eval_workspace_bytes()), dtype=torch.uint8, device="cuda")
    out3 = torch.full((3,), float(SENTINEL), dtype=torch.float64, device="cuda")
    ip_d, idx_d, val_d = _dev(indptr, np.int64), _dev(indices, np.int32), _dev(values, np.float32)
    _lib.check(lib.wmf_eval_sqerr(_ptr(Ud), _ptr(Id), f, ld, bias, _ptr(ip_d), _ptr(idx_d), _ptr(val_d), n, _ptr(out3), _ptr(ws), _stream()))
    return out3.cpu().numpy()


def _hits(Ud, Id, f, ld, bias, pair_user, pair_item, pair_row, cand, slot, topn, prefill=7, n_pairs=None):
    _lib, lib, _ptr, _stream = _api()
    cand = np.asarray(cand, dtype=np.int32)
    n_pairs = len(pair_row) if n_pairs is None else n_pairs
    hits = torch.full((len(topn),), prefill, dtype=torch.int64, device="cuda")
    pu_d, pi_d, pr_d, cand_d, slot_d, topn_d = (_dev(a, np.int32) for a in (pair_user, pair_item, pair_row, cand, slot, topn))
    _lib.check(lib.wmf_hit_counts(_ptr(Ud), _ptr(Id), f, ld, bias, _ptr(pu_d), _ptr(pi_d), _ptr(pr_d), n_pairs, _ptr(cand_d), cand.shape[1],
                                  _ptr(slot_d), _ptr(topn_d), len(topn), _ptr(hits), _stream()))
    return hits.cpu().numpy()


class _Rank:
    """wmf_rank_topn for one candidate list: the list and the workspace go to the device once."""

    def __init__(self, Ud, Id, f, ld, bias, cand):
        self.args, self.n = (Ud, Id, f, ld, bias), len(cand)
        self.cand = _dev(cand, np.int32)
        self.ws = torch.empty(int(_api()[1].wmf_rank_workspace_bytes(self.n)), dtype=torch.uint8, device="cuda")

    def __call__(self, user, topn, scores=True):
        _lib, lib, _ptr, _stream = _api()
        Ud, Id, f, ld, bias = self.args
        pos = torch.full((topn,), -1, dtype=torch.int32, device="cuda")
        sc = torch.full((topn,), SENTINEL, dtype=torch.float32, device="cuda") if scores else None
        user_d = _dev([user], np.int32)
        _lib.check(lib.wmf_rank_topn(_ptr(Ud), _ptr(Id), f, ld, bias, _ptr(user_d), _ptr(self.cand), self.n, topn,
                                     _ptr(pos), _ptr(sc), _ptr(self.ws), self.ws.numel(), _stream()))
        return pos.cpu().numpy(), (sc.cpu().numpy() if scores else None)


class _RankBatch:
    """wmf_rank_topn_batch over prefixes of one user list and one candidate list."""

    def __init__(self, Ud, Id, f, ld, bias, users, cand):
        self.args = (Ud, Id, f, ld, bias)
        self.users, self.cand = _dev(np.append(users, users[:1]), np.int32), _dev(np.append(cand, cand[:1]), np.int32)   # (one spare each)
        self.ws = torch.empty(int(_api()[1].wmf_rank_batch_workspace_bytes(len(users), len(cand))), dtype=torch.uint8, device="cuda")

    def __call__(self, nu, nc, topn, scores=True):
        _lib, lib, _ptr, _stream = _api()
        Ud, Id, f, ld, bias = self.args
        assert int(lib.wmf_rank_batch_workspace_bytes(nu, nc)) <= self.ws.numel()
        pos = torch.full((nu, topn), -1, dtype=torch.int32, device="cuda")
        sc = torch.full((nu, topn), SENTINEL, dtype=torch.float32, device="cuda") if scores else None
        _lib.check(lib.wmf_rank_topn_batch(_ptr(Ud), _ptr(Id), f, ld, bias, _ptr(self.users), nu, _ptr(self.cand), nc, topn, _ptr(pos),
                                           _ptr(sc), _ptr(self.ws), self.ws.numel(), _stream()))
        return pos.cpu().numpy(), (sc.cpu().numpy() if scores else None)


def _check_rounded_order(pos, ref_scores, bound, what):
    """Positions are unique and the reference score of the k-th returned candidate is within B of the k-th best reference
    score (B of whichever of the two candidates has the larger one).  Returns the worst ratio."""
    assert len(np.unique(pos)) == len(pos) and pos.min() >= 0 and pos.max() < len(ref_scores), what
    best = ref.stable_topn(ref_scores, len(pos))
    gap = np.abs(ref_scores[pos] - ref_scores[best])
    allowed = np.maximum(bound[pos], bound[best])
    ratio = float((gap / allowed).max())
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ----------------------------------------------------------------------------------------------------- 1. wmf_predict_pairs
def _predict_both_classes(f, bias, ld, ui, ii):
    """Exact class bit for bit, rounded class within B; returns the worst err / B."""
    Ue, Ie = _host(f, "exact")
    got = _predict(*_device(f, ld, "exact"), f, ld, bias, ui, ii)
    want = ref.scores_int(Ue, Ie, ui, ii, bias)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.rint(got)), \
        (f, bias, ld, len(ui), len(ii), np.flatnonzero(got != want)[:5])
    Un, In = _host(f, "rounded")
    got = _predict(*_device(f, ld, "rounded"), f, ld, bias, ui, ii).astype(np.float64)
    err = np.abs(got - ref.scores_f64(Un, In, ui, ii, bias))
    ratio = float((err / ref.score_bound(Un, In, ui, ii, bias)).max())
    assert ratio <= 1.0, (f, bias, ld, len(ui), len(ii), ratio)
    return ratio


@case
def test_predict_pairs(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(100 + 2 * f + bias)
    ui, ii = rng.integers(0, N_USERS, 1000), rng.integers(0, N_ITEMS, 1000)
    ui[:40], ii[20:60] = ui[0], ii[20]                              # runs of one user, of one item, of one pair
    worst = 0.0
    for us, its in ((ui, ii), (ui[5:6], ii), (ui, ii[7:8]), (ui[9:10], ii[9:10])):   # pairwise, one user, one item, n = 1
        worst = max(worst, _predict_both_classes(f, bias, ld, us, its))
    _record("predict_kernel", f, bias, ld, worst)


@pytest.mark.parametrize("bias", (0, 1))
def test_predict_pairs_beyond_the_grid_cap(bias):
    """More than 8192 x 16 pairs: the grid-stride loop takes a second trip."""
    f, n = 5, 8192 * 16 + 9001
    rng = np.random.default_rng(3)
    ui, ii = rng.integers(0, N_USERS, n), rng.integers(0, N_ITEMS, n)
    _predict_both_classes(f, bias, _ld(f), ui, ii)
    _predict_both_classes(f, bias, _ld(f), ui[:1], ii)


def test_predict_pairs_with_an_empty_side_writes_nothing():
    """n_u = 0 against n_i = 1 (or the reverse, or both empty) is no pair at all: OK, and the output is left alone.  Every
    buffer handed over is valid and has one element or more."""
    _lib, lib, _ptr, _stream = _api()
    f, ld = 5, _ld(5)
    Ud, Id = _device(f, ld, "exact")
    one = _dev([0], np.int32)
    for n_u, n_i in ((0, 1), (1, 0), (0, 0)):
        out = torch.full((4,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(lib.wmf_predict_pairs(_ptr(Ud), _ptr(Id), f, ld, 1, _ptr(one), n_u, _ptr(one), n_i, _ptr(out), _stream()))
        assert (out.cpu().numpy() == np.float32(SENTINEL)).all(), (n_u, n_i)
    two = _dev([0, 1], np.int32)                                    # lengths that fit neither form are still refused
    assert lib.wmf_predict_pairs(_ptr(Ud), _ptr(Id), f, ld, 1, _ptr(two), 0, _ptr(two), 2, _ptr(out), _stream()) == _lib.WMF_EINVAL


# -------------------------------------------------------------------------------------------------------- 2. wmf_eval_sqerr
def _eval_csr(rng, n_rows, fixed_degrees, max_random_degree):
    deg = np.concatenate([fixed_degrees, rng.integers(0, max_random_degree + 1, n_rows - len(fixed_degrees))]).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    # a row of N_ITEMS entries holds every item once, in random order; the others draw with replacement (duplicates are kept)
    indices = np.concatenate([rng.permutation(N_ITEMS) if d == N_ITEMS else rng.integers(0, N_ITEMS, d) for d in deg] + [[0]])
    return deg, indptr, indices[:indptr[-1] + 1]                  # (one spare element: never an empty buffer)


@case
def test_eval_sqerr(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(200 + 2 * f + bias)
    deg, indptr, indices = _eval_csr(rng, N_USERS, [0, 1, 2, 3, 4, 5, 9, N_ITEMS, 0, N_ITEMS], 12)
    nnz, rows = int(indptr[-1]), ref.csr_rows(indptr)
    # exact class: integer values, stored 0.0 and -0.0 among them; the sums are integers below 2^53 in any order
    values = np.append(rng.integers(-5, 6, nnz).astype(np.float32), 1.0)
    values[rng.choice(nnz, 25, replace=False)] = -0.0
    assert (values[:nnz] == 0).sum() > 30 and np.signbit(values[:nnz]).sum() > 25
    Ue, Ie = _host(f, "exact")
    want = ref.eval_sums(ref.scores_int(Ue, Ie, rows, indices[:nnz], bias), values[:nnz])
    got = _eval(*_device(f, ld, "exact"), f, ld, bias, indptr, indices, values, N_USERS)
    assert got.tolist() == [float(x) for x in want], (f, bias, ld, got, want)
    # only stored zeros: nothing is counted
    zeros = np.where(np.arange(nnz + 1) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    assert _eval(*_device(f, ld, "exact"), f, ld, bias, indptr, indices, zeros, N_USERS).tolist() == [0.0, 0.0, 0.0]
    # no rows
    assert _eval(*_device(f, ld, "exact"), f, ld, bias, [0], [0], [1.0], 0).tolist() == [0.0, 0.0, 0.0]
    # rounded class: the float64 sums of the device's own scores for the same entries (those are bounded in test_predict_pairs);
    # the arithmetic is the same, the order of the double summation is not
    values = np.append(rng.standard_normal(nnz).astype(np.float32), 1.0)
    values[::11], values[5::11] = 0.0, -0.0
    Ud, Id = _device(f, ld, "rounded")
    scores = _predict(Ud, Id, f, ld, bias, rows, indices[:nnz])
    sq, ab, cnt = ref.eval_sums(scores.astype(np.float64), values[:nnz])
    got = _eval(Ud, Id, f, ld, bias, indptr, indices, values, N_USERS)
    assert got[2] == cnt and 0 < cnt < nnz
    np.testing.assert_allclose(got[:2], [sq, ab], rtol=1e-12, atol=0)


@pytest.mark.parametrize("bias", (0, 1))
def test_eval_sqerr_beyond_the_grid_cap(bias):
    """More than 2048 x 4 user rows: the row loop takes a second trip, and every partial block is summed."""
    f, n_rows = 5, 2048 * 4 + 811
    ld = _ld(f)
    rng = np.random.default_rng(4)
    deg, indptr, indices = _eval_csr(rng, n_rows, [], 6)
    nnz, rows = int(indptr[-1]), ref.csr_rows(indptr)
    values = np.append(rng.integers(-5, 6, nnz).astype(np.float32), 1.0)
    Ue, Ie = _host(f, "exact", n_rows)
    want = ref.eval_sums(ref.scores_int(Ue, Ie, rows, indices[:nnz], bias), values[:nnz])
    got = _eval(*_device(f, ld, "exact", n_rows), f, ld, bias, indptr, indices, values, n_rows)
    assert got.tolist() == [float(x) for x in want]
    assert deg[-400:].sum() > 0                                     # the rows of the second trip hold entries


# -------------------------------------------------------------------------------------------------------- 3. wmf_hit_counts
N_CANDS = (1, 2, 3, 4, 5, 7, 64, 101)


def _hit_case(rng, n_pairs, n_rows, n_cand):
    """Test entries that share candidate rows; slots at 0, in the middle and at the end; the test item of some entries once
    more elsewhere in its row (a tie, which is not "higher"); whatever sits AT the slot is not a candidate."""
    pair_user, pair_item = rng.integers(0, N_USERS, n_pairs), rng.integers(0, N_ITEMS, n_pairs)
    pair_row = rng.integers(0, n_rows, n_pairs)
    cand = rng.integers(0, N_ITEMS, (n_rows, n_cand))
    slot = np.array([0, n_cand // 2, n_cand - 1])[np.arange(n_rows) % 3]
    for p in range(0, min(n_pairs, 4 * n_rows), 3):
        j = (slot[pair_row[p]] + 1 + p) % n_cand
        if j != slot[pair_row[p]]:
            cand[pair_row[p], j] = pair_item[p]
    return pair_user, pair_item, pair_row, cand, slot


def _topn_lists(rng, n_cand):
    wide = rng.integers(0, n_cand + 3, 64)
    wide[:5] = (0, 1, n_cand, n_cand + 1, n_cand - 1)
    return ([1], [0, n_cand, n_cand + 5], wide.tolist())


@case
def test_hit_counts(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(300 + 2 * f + bias)
    M = _matrix(f, bias)
    Ud, Id = _device(f, ld, "exact")
    seen_tie = seen_hit = seen_miss = False
    for n_cand in N_CANDS:
        pu, pi, pr, cand, slot = _hit_case(rng, 60, 12, n_cand)
        s_true, s_cand = M[pu, pi], M[pu[:, None], cand[pr]]
        seen_tie |= bool(((s_cand == s_true[:, None]) & (np.arange(n_cand)[None, :] != slot[pr][:, None])).any())
        for topn in _topn_lists(rng, n_cand):
            want = ref.hit_counts(s_true, s_cand, slot[pr], topn)
            got = _hits(Ud, Id, f, ld, bias, pu, pi, pr, cand, slot, topn)
            assert np.array_equal(got, want), (f, bias, ld, n_cand, topn, got, want)
            seen_hit |= bool((want > 0).any())
            seen_miss |= bool((want < 60).any())
    assert seen_tie and seen_hit and seen_miss
    # no test entries: the counts are cleared, whatever they held
    one = np.zeros(1, dtype=np.int32)
    assert _hits(Ud, Id, f, ld, bias, one, one, one, one[None, :], one, [1, 2, 3], prefill=-99, n_pairs=0).tolist() == [0, 0, 0]
    # rounded class: the counts the host derives from wmf_predict_pairs scores of the same pairs -- exactly, which holds only
    # because hit_kernel (csrc/wmf_rank.hip) and predict_kernel (csrc/wmf_eval.hip) score with the one wmf_pair_score
    Ud, Id = _device(f, ld, "rounded")
    pu, pi, pr, cand, slot = _hit_case(rng, 60, 12, 101)
    s_true = _predict(Ud, Id, f, ld, bias, pu, pi)
    s_cand = _predict(Ud, Id, f, ld, bias, np.repeat(pu, 101), cand[pr].ravel()).reshape(60, 101)
    topn = _topn_lists(rng, 101)[2]
    got = _hits(Ud, Id, f, ld, bias, pu, pi, pr, cand, slot, topn)
    assert np.array_equal(got, ref.hit_counts(s_true, s_cand, slot[pr], topn)), (f, bias, ld)


def test_hit_counts_beyond_the_grid_cap():
    """More than 16384 x 4 test entries (five candidates each)."""
    f, bias, n_pairs, n_rows, n_cand = 5, 1, 16384 * 4 + 4467, 500, 5
    ld = _ld(f)
    rng = np.random.default_rng(5)
    M = _matrix(f, bias)
    pu, pi, pr, cand, slot = _hit_case(rng, n_pairs, n_rows, n_cand)
    topn = [0, 1, 2, 3, 4, 5]
    want = ref.hit_counts(M[pu, pi], M[pu[:, None], cand[pr]], slot[pr], topn)
    got = _hits(*_device(f, ld, "exact"), f, ld, bias, pu, pi, pr, cand, slot, topn)
    assert np.array_equal(got, want) and want[0] == 0 and want[-1] == n_pairs and (np.diff(want) > 0).all()


# --------------------------------------------------------------------------------------------------------- 4. wmf_rank_topn
RANK_N_CAND = (1, 2, 255, 256, 257, 5000)


def _topns(n):
    return sorted({1, max(1, n // 2), max(1, n - 1), n})


@case
def test_rank_topn(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(400 + 2 * f + bias)
    M = _matrix(f, bias)
    Un, In = _host(f, "rounded")
    worst = 0.0
    for n_cand in RANK_N_CAND:
        cand = rng.integers(0, N_ITEMS, n_cand)                      # duplicates from the third list on: real ties
        user = int(rng.integers(0, N_USERS))
        # exact class: the stable descending order, position by position, and the scores
        rank = _Rank(*_device(f, ld, "exact"), f, ld, bias, cand)
        scores = M[user, cand]
        for topn in _topns(n_cand):
            want = ref.stable_topn(scores, topn)
            pos, sc = rank(user, topn, scores=(topn != n_cand or n_cand != 257))      # (once without out_scores)
            assert np.array_equal(pos, want), (f, bias, ld, n_cand, topn, np.flatnonzero(pos != want)[:5])
            assert sc is None or np.array_equal(sc.astype(np.int64), scores[want]), (f, bias, ld, n_cand, topn)
        # rounded class
        Ud, Id = _device(f, ld, "rounded")
        rank = _Rank(Ud, Id, f, ld, bias, cand)
        ref_scores = ref.scores_f64(Un, In, [user], cand, bias)
        bound = ref.score_bound(Un, In, [user], cand, bias)
        dev_scores = _predict(Ud, Id, f, ld, bias, [user], cand)
        for topn in _topns(n_cand):
            pos, sc = rank(user, topn)
            worst = max(worst, _check_rounded_order(pos, ref_scores, bound, (f, bias, ld, n_cand, topn)))
            assert np.array_equal(sc.view(np.uint32), dev_scores[pos].view(np.uint32)), (f, bias, ld, n_cand, topn)
            assert np.array_equal(pos, ref.stable_topn(dev_scores, topn))            # the device's own scores, in its stable order
    _record("rank_topn_order", f, bias, ld, worst)


def test_rank_topn_beyond_the_grid_cap():
    """600 000 candidates, more than the 2048 x 256 the histogram and the compaction cover in one trip."""
    f, bias, n_cand = 5, 1, 600_000
    ld = _ld(f)
    rng = np.random.default_rng(6)
    cand = rng.integers(0, N_ITEMS, n_cand)
    rank = _Rank(*_device(f, ld, "exact"), f, ld, bias, cand)
    scores = _matrix(f, bias)[11, cand]
    order = ref.stable_topn(scores, n_cand)
    for topn in (10, n_cand):
        pos, sc = rank(11, topn)
        assert np.array_equal(pos, order[:topn]) and np.array_equal(sc.astype(np.int64), scores[order[:topn]]), topn
    assert (order[:10] < 2048 * 256).all() and n_cand > 2048 * 256  # ties: the ten best are early ones; now a late winner
    row = _matrix(f, bias)[12]
    cand[row[cand] == row.max()] = int(np.argmin(row))              # the best score occurs once, in the second trip
    cand[-7] = int(np.argmax(row))
    rank = _Rank(*_device(f, ld, "exact"), f, ld, bias, cand)
    scores = _matrix(f, bias)[12, cand]
    pos, sc = rank(12, 1000)
    want = ref.stable_topn(scores, 1000)
    assert np.array_equal(pos, want) and np.array_equal(sc.astype(np.int64), scores[want]) and want[0] == n_cand - 7


def test_rank_topn_cut_on_every_histogram_boundary():
    """f = 1 and a user factor of 1.0: score = item value.  Score levels that share a bin of the select's histogram, that sit
    in two bins of one 16-bin group, in different groups and in group 0; topn at every cumulative count of the levels and one
    to either side, so the cut falls exactly on a bin boundary, a group boundary, and reaches down to group 0."""
    _lib, lib, _ptr, _stream = _api()
    values, levels, counts = ref.hist_case(0)
    assert all(ref.hist_bin_properties(levels).values())
    n, ld = len(values), _ld(1)
    Ud = _dev(ref.padded(np.ones((1, 1), dtype=np.float32), ld))
    Id = _dev(ref.padded(values[:, None], ld))
    rank = _Rank(Ud, Id, 1, ld, 0, np.arange(n))
    order = ref.stable_topn(values, n)
    cum = np.cumsum(counts[::-1])                                    # candidates at or above each level, best level first
    assert cum[-1] == n
    for topn in sorted({int(t) for c in cum for t in (c - 1, c, c + 1) if 1 <= t <= n}):
        pos, sc = rank(0, topn)
        assert np.array_equal(pos, order[:topn]), (topn, np.flatnonzero(pos != order[:topn])[:5])
        assert np.array_equal(sc.view(np.uint32), values[order[:topn]].view(np.uint32)), topn


# --------------------------------------------------------------------------------------------------- 5. wmf_rank_topn_batch
BATCH_USERS, BATCH_CANDS = (1, 15, 16, 17, 33), (1, 15, 16, 17, 31, 33, 257)


@case
def test_rank_topn_batch(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(500 + 2 * f + bias)
    users, cand = rng.integers(0, N_USERS, 33), rng.integers(0, N_ITEMS, 257)
    users[5], cand[9], cand[200] = users[2], cand[3], cand[3]      # a user twice, a candidate three times
    M = _matrix(f, bias)[users[:, None], cand[None, :]]
    Un, In = _host(f, "rounded")
    R = ref.scores_f64(Un, In, np.repeat(users, 257), np.tile(cand, 33), bias).reshape(33, 257)
    B = ref.score_bound(Un, In, np.repeat(users, 257), np.tile(cand, 33), bias).reshape(33, 257)
    exact = _RankBatch(*_device(f, ld, "exact"), f, ld, bias, users, cand)
    rounded = _RankBatch(*_device(f, ld, "rounded"), f, ld, bias, users, cand)
    worst_score = worst_order = 0.0
    for nu in BATCH_USERS:
        for nc in BATCH_CANDS:
            what = (f, bias, ld, nu, nc)
            want = np.stack([ref.stable_topn(M[u, :nc], nc) for u in range(nu)])
            for topn, scores in ((nc, True), (1, True), (1 if (nu + nc) % 2 else nc, False)):
                pos, sc = exact(nu, nc, topn, scores)
                assert np.array_equal(pos, want[:, :topn]), (what, topn, scores)
                assert sc is None or np.array_equal(sc.astype(np.int64), np.take_along_axis(M[:nu, :nc], want[:, :topn], axis=1)), (what, topn)
            for topn in (nc, 1):
                pos, sc = rounded(nu, nc, topn)
                assert pos.min() >= 0 and pos.max() < nc, what
                err = np.abs(sc.astype(np.float64) - np.take_along_axis(R[:nu, :nc], pos.astype(np.int64), axis=1))
                worst_score = max(worst_score, float((err / np.take_along_axis(B[:nu, :nc], pos.astype(np.int64), axis=1)).max()))
                assert (np.diff(sc, axis=1) <= 0).all(), what           # best first, by the device's own scores
                for u in range(nu):
                    worst_order = max(worst_order, _check_rounded_order(pos[u], R[u, :nc], B[u, :nc], (what, topn, u)))
    assert worst_score <= 1.0, (f, bias, ld, worst_score)
    _record("score_tile_kernel", f, bias, ld, worst_score)
    _record("rank_topn_batch_order", f, bias, ld, worst_order)
    # exact class, user by user: the batched call and the one-user call agree
    one = _Rank(*_device(f, ld, "exact"), f, ld, bias, cand)
    pos, sc = exact(17, 257, 257)
    for u in range(17):
        p1, s1 = one(int(users[u]), 257)
        assert np.array_equal(pos[u], p1) and np.array_equal(sc[u], s1), (f, bias, ld, u)


def test_rank_topn_batch_beyond_the_grid_cap():
    """48 users x 400 000 candidates: 75 000 score tiles, more than the 16384 x 4 of one trip."""
    f, bias, nu, nc, topn = 5, 1, 48, 400_000, 10
    ld = _ld(f)
    rng = np.random.default_rng(7)
    users, cand = rng.integers(0, N_USERS, nu), rng.integers(0, N_ITEMS, nc)
    batch = _RankBatch(*_device(f, ld, "exact"), f, ld, bias, users, cand)
    pos, sc = batch(nu, nc, topn)
    del batch
    torch.cuda.empty_cache()
    M = _matrix(f, bias)
    for u in range(nu):
        scores = M[users[u], cand]
        want = ref.stable_topn(scores, topn)
        assert np.array_equal(pos[u], want) and np.array_equal(sc[u].astype(np.int64), scores[want]), u
    # a variant whose best candidates sit in the tiles of the second trip
    cand[:nc - 1000] = int(np.argmin(M[users[-1]]))
    cand[-3:] = np.argsort(-M[users[-1]], kind="stable")[:3]
    batch = _RankBatch(*_device(f, ld, "exact"), f, ld, bias, users, cand)
    pos, sc = batch(nu, nc, topn)
    want = ref.stable_topn(M[users[-1], cand], topn)
    assert np.array_equal(pos[-1], want) and want[0] >= nc - 1000  # user 47, last candidates: the last tile of all


# --------------------------------------------------------------------------------------------------------- 6. wmf_spmm_rows
def _spmm(Vd, f, ld, indptr, indices, values, n):
    _lib, lib, _ptr, _stream = _api()
    g = torch.full((max(n, 1), ld), SENTINEL, dtype=torch.float32, device="cuda")
    ip_d, idx_d, val_d = _dev(indptr, np.int64), _dev(indices, np.int32), _dev(values, np.float32)
    _lib.check(lib.wmf_spmm_rows(_ptr(Vd), _ptr(ip_d), _ptr(idx_d), _ptr(val_d), n, f, ld, _ptr(g), _stream()))
    return g.cpu().numpy()


def _spmm_ref(V, ld, indptr, indices, values):
    import scipy.sparse as sp
    n = len(indptr) - 1
    C = sp.csr_matrix((np.rint(values[:indptr[-1]]).astype(np.int64), indices[:indptr[-1]], indptr), shape=(n, V.shape[0]))
    return ref.padded(np.asarray((C @ np.rint(V).astype(np.int64))), ld, dtype=np.int64)


@pytest.mark.parametrize("f,extra", [(f, 0) for f in WIDTHS] + list(LD_EXTRA.items()))
def test_spmm_rows(f, extra):
    """Integer weights -3 .. 3 on integer rows -3 .. 3: |g| <= 9 * 300, exact in float32; the padding columns come back zero."""
    ld = _ld(f, extra)
    rng = np.random.default_rng(600 + f)
    deg, indptr, indices = _eval_csr(rng, 12, [0, 1, 5, N_ITEMS, 0, 5, N_ITEMS, 1], 9)
    values = np.append(rng.integers(-3, 4, indptr[-1]).astype(np.float32), 1.0)
    V = _host(f, "exact")[1]
    got = _spmm(_device(f, ld, "exact")[1], f, ld, indptr, indices, values, 12)
    want = _spmm_ref(V, ld, indptr, indices, values)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.rint(got)), (f, ld)
    assert (got[:, f:] == 0).all() and (got[deg == 0] == 0).all() and np.abs(want).max() > 9
    assert (_spmm(_device(f, ld, "exact")[1], f, ld, [0], [0], [1.0], 0) == np.float32(SENTINEL)).all()       # no rows: nothing written


def test_spmm_rows_beyond_the_grid_cap():
    """More than 8192 x 4 rows."""
    f, n = 5, 8192 * 4 + 1203
    ld = _ld(f)
    rng = np.random.default_rng(8)
    deg, indptr, indices = _eval_csr(rng, n, [], 3)
    values = np.append(rng.integers(-3, 4, indptr[-1]).astype(np.float32), 1.0)
    got = _spmm(_device(f, ld, "exact")[1], f, ld, indptr, indices, values, n)
    want = _spmm_ref(_host(f, "exact")[1], ld, indptr, indices, values)
    assert np.array_equal(got.astype(np.int64), want) and np.abs(want[-1000:]).max() > 0


# ------------------------------------------------------------------------------------------------------- 7. wmf_gather_rows
def _gather(src, ld, rows, n):
    _lib, lib, _ptr, _stream = _api()
    out = torch.full((max(n, 1), ld), SENTINEL, dtype=torch.float32, device="cuda")
    rows_d = _dev(rows, np.int64)
    _lib.check(lib.wmf_gather_rows(_ptr(src), ld, _ptr(rows_d), n, _ptr(out), _stream()))
    torch.cuda.synchronize()                                        # rows_d lives until the kernel has run
    return out


@pytest.mark.parametrize("ld", (4, 68, 132, 272))
def test_gather_rows(ld):
    """Bit-equal rows: the source holds arbitrary bit patterns (NaNs and denormals among them)."""
    rng = np.random.default_rng(700 + ld)
    bits = rng.integers(0, 2 ** 32, (500, ld), dtype=np.uint64).astype(np.uint32)
    src = _dev(bits.view(np.float32))
    for n in (1, 3, 64, 777):
        rows = rng.integers(0, 500, n)
        rows[: n // 3] = rows[0]                                      # repeated, unsorted
        got = _gather(src, ld, rows, n).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, bits[rows]), (ld, n)
    assert (_gather(src, ld, [0], 0).cpu().numpy() == np.float32(SENTINEL)).all()       # n = 0: nothing written


def test_gather_rows_beyond_the_grid_cap():
    """70 000 rows of 68 pieces: more than 16384 x 256 pieces."""
    ld, n = 272, 70_000
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2 ** 32, (500, ld), dtype=np.uint64).astype(np.uint32)
    rows = rng.integers(0, 500, n)
    src = _dev(bits.view(np.float32))
    got = _gather(src, ld, rows, n)
    want = src.view(torch.int32)[_dev(rows, np.int64)]
    assert torch.equal(got.view(torch.int32), want)
    assert np.array_equal(got[-5:].cpu().numpy().view(np.uint32), bits[rows[-5:]])


# ------------------------------------------------------------------------------------------------ 8. confidence transforms
CONF_LENGTHS = (1, 255, 256, 257, 4096 * 256 + 3)
CONF_PARAMS = ((10.0, 1.0), (2.5, 0.5), (-40.0, 0.25))              # exact in float32: the kernel's cast of alpha, beta costs nothing


def _conf_values(n, dtype):
    rng = np.random.default_rng(n)
    x = (rng.integers(0, 50, n) * rng.random(n)).astype(dtype)
    special = np.array([0, 1e-6, 1, 5, 1e6], dtype=dtype)
    x[: min(n, 5)] = special[: min(n, 5)]
    x[-min(n, 5):] = special[: min(n, 5)]                            # ... and in the last trip of the loop
    return x


@pytest.mark.parametrize("n", CONF_LENGTHS)
def test_confidence_transform(n):
    """float32: |err| <= |alpha| 2^-23 + 4 x 2^-24 |result| against float64 on the float32 inputs -- one rounding of 1 + beta x
    (fused or not) carried through the log, then logf and the product; float64: the same with 2^-52, 2^-53 against long double.
    alpha x (mode 1) is one rounding: 2^-24 |result| (2^-53)."""
    _lib, lib, _ptr, _stream = _api()
    for dtype, wide, u, fn in ((np.float32, np.float64, 2.0 ** -24, lib.wmf_confidence_transform),
                               (np.float64, np.longdouble, 2.0 ** -53, lib.wmf_confidence_transform_f64)):
        x = _conf_values(n, dtype)
        xw = x.astype(wide)
        for alpha, beta in CONF_PARAMS:
            for mode in (0, 1):
                d = _dev(x)
                _lib.check(fn(_ptr(d), n, alpha, beta, mode, _stream()))
                got = d.cpu().numpy().astype(wide)
                want = wide(alpha) * np.log1p(wide(beta) * xw) if mode == 0 else wide(alpha) * xw
                bound = abs(alpha) * 2 * u + 4 * u * np.abs(want) if mode == 0 else u * np.abs(want)
                err = np.abs(got - want)
                assert (err <= bound).all(), (dtype.__name__, n, alpha, beta, mode, float((err / np.maximum(bound, 1e-300)).max()))
                ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
                record_error(f"serving_confidence_{dtype.__name__}", **{f"n{n}_alpha{alpha}_beta{beta}_mode{mode}": ratio})


# ------------------------------------------------------------------------- 9. training's metric and the padding invariant
ENGINE_CASES = [(50, 0, None), (64, 1, None), (100, 0, None), (128, 1, None), (128, 1, "0"), (208, 1, None), (256, 1, None)]


@pytest.mark.parametrize("k,bias,rolled", ENGINE_CASES, ids=[f"k{k}-b{b}" + ("-unrolled" if r else "") for k, b, r in ENGINE_CASES])
def test_engine_padding_is_zero_and_eval_sums_match_the_oracle(k, bias, rolled, monkeypatch):
    """The evaluation kernels sum all ld columns of a row: they are right only while the solvers write the padding columns
    [f, ld) as exact zeros (include/wmf_hip.h).  After a half step on each side the padding IS zero, and the engine's own
    metric agrees with the oracle's eval_prec on the factors it reports."""
    import scipy.sparse as sp
    from oracle import wmf_oracle as orc
    from recmodel_amd import WMF
    from recmodel_amd.engine import AlsEngine
    if rolled is not None:
        monkeypatch.setenv("WMF_ROLLED", rolled)
    else:
        monkeypatch.delenv("WMF_ROLLED", raising=False)
    n_rows, m_fixed = 300, 2000
    rng = np.random.default_rng(900 + k)
    deg = rng.integers(1, 61, n_rows)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.concatenate([np.sort(rng.choice(m_fixed, d, replace=False)) for d in deg]).astype(np.int64)
    w = (10 * np.log(1 + rng.integers(1, 8, indptr[-1]))).astype(np.float32)
    w[rng.random(w.size) < 0.02] = 0.0
    eng = AlsEngine(n_rows, m_fixed, k, bias, 0.1)
    assert eng.rolled == (k == 128 and rolled is None)
    eng.set_interactions(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(w).cuda())
    Y = WMF(num_items=m_fixed, num_users=1, dim=k, gamma=0.1, weighted=True, bias=bool(bias), seed=k).items
    eng.set_factors("items", Y)
    eng.half_step("users")
    eng.half_step("items")
    eng.check_numerics()
    f, ld = eng.f, eng.ld
    assert f == k + bias and ld == _ld(f)
    for side in ("users", "items"):
        blk = eng.factors[side]
        assert blk.shape[1] == ld and bool((blk[:, f:] == 0).all()), side
        assert bool(torch.isfinite(blk).all()) and float(blk[:, :f].abs().max()) > 0
    assert bool((eng.X["items"][:, f:] == 0).all())
    # a utility matrix of its own, stored zeros among the entries
    deg_e = rng.integers(0, 9, n_rows)
    ip_e = np.concatenate([[0], np.cumsum(deg_e)])
    idx_e = np.concatenate([np.sort(rng.choice(m_fixed, d, replace=False)) for d in deg_e]).astype(np.int64)
    val_e = rng.integers(0, 6, ip_e[-1]).astype(np.float32)
    assert 0 < (val_e == 0).sum() < len(val_e)
    shard = eng.make_eval_shard(torch.from_numpy(ip_e), torch.from_numpy(idx_e), torch.from_numpy(val_e))
    sq, ab, cnt = eng.eval_sums(shard)
    Uf, If = eng.get_factors("users").astype(np.float64), eng.get_factors("items").astype(np.float64)
    mat = sp.csr_matrix((val_e.astype(np.float64), idx_e, ip_e), shape=(n_rows, m_fixed))
    assert cnt == float((val_e != 0).sum())
    np.testing.assert_allclose(sq / cnt, orc.eval_prec(Uf, If, mat, bool(bias), "mse"), rtol=1e-5, atol=0)
    np.testing.assert_allclose(ab / cnt, orc.eval_prec(Uf, If, mat, bool(bias), "mae"), rtol=1e-5, atol=0)
