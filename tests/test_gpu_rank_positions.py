"""wmf_rank_positions through the C ABI, per element (csrc/wmf_rankpos.hip): the exact place of every target item of a row in the
full-catalogue order of wmf_recommend_topn, the row's seen items left out -- target keys by a diagonal MFMA tile, one counting
scan of the catalogue (integer buckets, the catalogue cut into slices), the seen items taken off by a small third pass.

The vocabulary of tests/test_gpu_recommend.py: the same widths, bias settings and leading dimensions, the same two input classes
(tests/serving_ref.py) -- EXACT, integers, where the device must equal tests/rankpos_ref.py bit for bit and equal scores are real
ties, and ROUNDED, standard normal, held by two derived conditions and no tolerance: the defining property against
wmf_recommend_topn on the same device buffers, and the interval the float64 scores and their bound B(u, i) leave for the rank.
Shapes are the smallest at which the kernels can go wrong: row counts around the 16 users of a wave, catalogue lengths around the
16-item tile and the stage, every slice count from one to more slices than tiles, target counts around the per-row limit."""
import numpy as np
import pytest
import torch

import rankpos_ref as pref
import recommend_ref as rref
import serving_ref as ref
from scan_cases import N_ITEMS, N_PATTERNS, N_USERS, _api, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list, case

pytestmark = pytest.mark.gpu

GRID_ROWS, GRID_ITEMS, GRID_SLICES = (1, 15, 16, 17, 33, 40), (1, 15, 16, 17, 255, 256, 257, 300), (0, 1, 2, 3, 7, 64)
RANK_SENTINEL, SCORE_SENTINEL = -777, -12345.0
LEAD, TAIL = 3, 5                                                  # untouched entries before the first and after the last target
MAX_T = _constant("WMF_RANKPOS_MAX_TARGETS", "include/wmf_hip.h")


# ------------------------------------------------------------------------------------------------------------------ helpers
class _Device:
    """wmf_rank_positions and wmf_recommend_topn on prefixes of one user list and of one item matrix, on the same device buffers."""

    def __init__(self, Uf, If, f, ld, bias, user_idx):
        self.Ud, self.Id, self.args = _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld)), (f, ld, bias)
        self.user_idx = _dev(user_idx, np.int32)

    def _seen(self, seen, n_rows):
        if seen is None:
            return None, None
        indptr, indices = rref.csr_of(seen)
        assert len(indptr) == n_rows + 1
        return _dev(indptr, np.int64), _dev(indices, np.int32)

    def positions(self, n_rows, n_items, n_slices, targets, seen=None, scores=True):
        """(ranks, scores) of all targets in row order; the entries around them must come back untouched."""
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        indptr, indices = rref.csr_of(targets)
        assert len(indptr) == n_rows + 1
        n = int(indptr[-1])
        tp_d = _dev(indptr + LEAD, np.int64)
        ti_d = _dev(np.concatenate([np.zeros(LEAD), indices[:n], np.zeros(TAIL)]), np.int32)
        ws = torch.empty(int(lib.wmf_rank_positions_workspace_bytes(n_rows, n, n_slices)), dtype=torch.uint8, device="cuda")
        rank = torch.full((LEAD + n + TAIL,), RANK_SENTINEL, dtype=torch.int32, device="cuda")
        sc = torch.full((LEAD + n + TAIL,), SCORE_SENTINEL, dtype=torch.float32, device="cuda") if scores else None
        ip_d, idx_d = self._seen(seen, n_rows)
        _lib.check(lib.wmf_rank_positions(_ptr(self.Ud), _ptr(self.Id), f, ld, bias, _ptr(self.user_idx), n_rows, n_items, _ptr(ip_d),
                                          _ptr(idx_d), _ptr(tp_d), _ptr(ti_d), n_slices, _ptr(rank), _ptr(sc), _ptr(ws), ws.numel(), _stream()))
        rank = rank.cpu().numpy()
        assert (rank[:LEAD] == RANK_SENTINEL).all() and (rank[LEAD + n:] == RANK_SENTINEL).all()
        if scores:
            sc = sc.cpu().numpy()
            assert (sc[:LEAD] == SCORE_SENTINEL).all() and (sc[LEAD + n:] == SCORE_SENTINEL).all()
        return rank[LEAD: LEAD + n], (sc[LEAD: LEAD + n] if scores else None)

    def recommend(self, n_rows, n_items, topn, n_slices, seen=None):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        ws = torch.empty(int(lib.wmf_recommend_workspace_bytes(n_rows, topn, n_slices)), dtype=torch.uint8, device="cuda")
        items = torch.full((n_rows, topn), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((n_rows, topn), SCORE_SENTINEL, dtype=torch.float32, device="cuda")
        ip_d, idx_d = self._seen(seen, n_rows)
        _lib.check(lib.wmf_recommend_topn(_ptr(self.Ud), _ptr(self.Id), f, ld, bias, _ptr(self.user_idx), n_rows, n_items, _ptr(ip_d),
                                          _ptr(idx_d), topn, n_slices, _ptr(items), _ptr(sc), None, _ptr(ws), ws.numel(), _stream()))
        return items.cpu().numpy(), sc.cpu().numpy()


def _target_rows(rng, user_scores, seen, n_items, kinds):
    """One target list per row.  Row b % 8 == 5 has none; rows 10, 11, 12 and 13 have MAX_T - 1, MAX_T, MAX_T + 1 and 2 MAX_T + 8
    random ones; every other row: the best and the worst eligible item, an item whose score ties with a lower and with a higher id,
    item n_items - 1, a seen item, and the first of them once more.  `kinds` collects what occurred."""
    rows = []
    for b, s in enumerate(user_scores):
        s = s[:n_items]
        if b % 8 == 5:
            rows.append(np.arange(0))
            kinds.add("none")
            continue
        if b in (10, 11, 12, 13):
            count = {10: MAX_T - 1, 11: MAX_T, 12: MAX_T + 1, 13: 2 * MAX_T + 8}[b]
            rows.append(rng.integers(0, n_items, count))
            kinds.add(("count", count))
            continue
        row = []
        elig = np.setdiff1d(np.arange(n_items), seen[b]) if seen is not None else np.arange(n_items)
        if len(elig):
            order = elig[ref.stable_topn(s[elig], len(elig))]
            row += [order[0], order[-1]]
            kinds.add("best and worst")
        values, counts = np.unique(s, return_counts=True)
        if (counts >= 3).any():
            tied = np.flatnonzero(s == values[np.argmax(counts >= 3)])
            row.append(tied[len(tied) // 2])
            kinds.add("tied both ways")
        row.append(n_items - 1)
        if seen is not None and len(seen[b]):
            row.append(seen[b][int(rng.integers(0, len(seen[b])))])
            kinds.add("seen")
        row.append(row[0])
        kinds.add("duplicate")
        rows.append(np.asarray(row, dtype=np.int64))
    return rows


def _want_exact(M, users, seen, targets, n_items):
    """(ranks, scores int64, counted) of all targets in row order: the reference for a row's first MAX_T targets, BEYOND after."""
    ranks, scores, counted = [], [], []
    for b, u in enumerate(users):
        t = np.asarray(targets[b], dtype=np.int64)
        head = pref.rank_positions_ref(M[u, :n_items], [] if seen is None else seen[b], t[:MAX_T])
        ranks.append(np.concatenate([head, np.full(max(len(t) - MAX_T, 0), pref.BEYOND)]))
        scores.append(M[u, t])
        counted.append(np.arange(len(t)) < MAX_T)
    return np.concatenate(ranks), np.concatenate(scores), np.concatenate(counted)


def _check_exact(got, want, what):
    (rank, sc), (want_rank, want_sc, counted) = got, want
    assert np.array_equal(rank, want_rank), (what, np.flatnonzero(rank != want_rank)[:5], rank[rank != want_rank][:5], want_rank[rank != want_rank][:5])
    assert np.array_equal(sc[counted].astype(np.int64), want_sc[counted]) and np.array_equal(sc[counted], np.rint(sc[counted])), what
    assert (sc[~counted] == SCORE_SENTINEL).all(), what            # a target past the limit is not scored


# ------------------------------------------------------------------------------------------- 1. EXACT: the grid, bit for bit
@case
def test_rank_positions_exact(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(3000 + 2 * f + bias)
    users = _user_list()
    M, _ = _scores(f, bias, "exact")
    dev = _Device(*_host(f, "exact"), f, ld, bias, users)
    patterns, kinds, beyond, seen_targets = set(), set(), 0, 0
    for ir, nr in enumerate(GRID_ROWS):
        for ii, ni in enumerate(GRID_ITEMS):
            seen = _seen_rows(rng, M[users[:nr]], ni, ir + ii)
            patterns |= {(b + ir + ii) % N_PATTERNS for b in range(nr)}
            targets = _target_rows(rng, M[users[:nr]], seen, ni, kinds)
            want = _want_exact(M, users[:nr], seen, targets, ni)
            first = None
            for n_slices in GRID_SLICES:
                got = dev.positions(nr, ni, n_slices, targets, seen)
                if first is None:
                    first = got
                    _check_exact(got, want, (f, bias, ld, nr, ni, n_slices))
                else:
                    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, first)), (f, bias, ld, nr, ni, n_slices)
            beyond += int((want[0] == pref.BEYOND).sum())
            seen_targets += int((want[0] == pref.SEEN).sum())
            if nr == N_USERS:                                       # seen_indptr = NULL, and once without scores
                targets = _target_rows(rng, M[users[:nr]], None, ni, kinds)
                want = _want_exact(M, users[:nr], None, targets, ni)
                got = dev.positions(nr, ni, GRID_SLICES[ii % len(GRID_SLICES)], targets, None)
                _check_exact(got, want, (f, bias, ld, nr, ni, "no seen list"))
                assert np.array_equal(dev.positions(nr, ni, 2, targets, None, scores=False)[0], got[0])
    assert patterns == set(range(N_PATTERNS)) and beyond and seen_targets
    assert kinds >= {"none", "best and worst", "tied both ways", "seen", "duplicate", ("count", MAX_T - 1), ("count", MAX_T), ("count", MAX_T + 1)}, kinds


# --------------------------------------------------------------------------------------------- 2. ROUNDED: derived conditions
def _rounded_targets(rng, s, seen_row, n_items):
    """Targets at the places where the property is decided -- the float64 best, the 10th and 11th, the 127th to 130th eligible
    item --, the worst, the last item, a seen item and random ones; at most MAX_T."""
    elig = np.setdiff1d(np.arange(n_items), seen_row)
    row = []
    if len(elig):
        order = elig[ref.stable_topn(s[elig], len(elig))]
        row += [order[k] for k in (0, 1, 9, 10, 126, 127, 128, 129) if k < len(order)] + [order[-1]]
    row.append(n_items - 1)
    if len(seen_row):
        row.append(seen_row[int(rng.integers(0, len(seen_row)))])
    row += list(rng.integers(0, n_items, MAX_T - len(row)))
    return np.asarray(row[:MAX_T], dtype=np.int64)


@case
def test_rank_positions_rounded(f, bias, extra):
    """Every target of every row: (a) 0 <= rank < k exactly when wmf_recommend_topn returns the target among its first k, with the
    same score bits, for k = 1, 10, 128; (b) the rank lies in the interval the float64 scores s and the bound B leave:
    #{eligible j: s_j - B_j > s_t + B_t} <= rank <= #{eligible j != t: s_j + B_j >= s_t - B_t}.  A seen target is SEEN."""
    ld = _ld(f, extra)
    rng = np.random.default_rng(5000 + 2 * f + bias)
    users = _user_list()
    R, B = _scores(f, bias, "rounded")
    dev = _Device(*_host(f, "rounded"), f, ld, bias, users)
    checked = hits = 0
    for ii, ni in enumerate((N_ITEMS, 257)):
        seen = _seen_rows(rng, R[users], ni, ii)
        targets = [_rounded_targets(rng, R[u, :ni], seen[b], ni) for b, u in enumerate(users)]
        rank, sc = dev.positions(N_USERS, ni, 0, targets, seen)
        again = dev.positions(N_USERS, ni, 3, targets, seen)
        assert np.array_equal(rank, again[0]) and np.array_equal(sc.view(np.uint32), again[1].view(np.uint32)), (f, bias, ld, ni)
        top_items, top_scores = dev.recommend(N_USERS, ni, 128, 0, seen)
        p = 0
        for b, u in enumerate(users):
            elig = np.ones(ni, dtype=bool)
            elig[seen[b]] = False
            s, bound = R[u, :ni], B[u, :ni]
            for t in targets[b]:
                what = (f, bias, ld, ni, b, int(t), int(rank[p]))
                assert abs(float(sc[p]) - s[t]) <= bound[t], what
                where = np.flatnonzero(top_items[b] == t)
                if not elig[t]:
                    assert rank[p] == pref.SEEN and len(where) == 0, what
                else:
                    for k in (1, 10, 128):
                        assert (0 <= rank[p] < k) == bool(len(where) and where[0] < k), (what, k)
                    if len(where):
                        assert rank[p] == where[0] and sc[p:p + 1].view(np.uint32)[0] == top_scores[b, where[0]:where[0] + 1].view(np.uint32)[0], what
                        hits += 1
                    low = int(((s - bound > s[t] + bound[t]) & elig).sum())
                    others = elig.copy()
                    others[t] = False
                    high = int(((s + bound >= s[t] - bound[t]) & others).sum())
                    assert low <= rank[p] <= high, (what, low, high)
                checked += 1
                p += 1
        assert p == len(rank)
    assert checked == sum(len(t) for t in targets) * 2 and hits > N_USERS


# ------------------------------------------------------------------------------------------------------ 3. the grid-stride caps
def test_rank_positions_beyond_the_scan_grid_cap():
    """More (user block, slice) pairs than workgroups of the scan, and more rows than the per-row kernels take in one trip: 17
    blocks of 64 rows x the largest slice count; the last block's only row is counted by the second trip."""
    f, bias = 5, 1
    n_slices = _constant("WMF_RECOMMEND_MAX_SLICES", "include/wmf_hip.h")
    cap = _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    n_rows = 64 * (cap // n_slices) + 1
    assert ((n_rows + 63) // 64) * n_slices > cap >= (n_rows // 64) * n_slices
    ld = _ld(f)
    M, _ = _scores(f, bias, "exact")
    users = np.arange(n_rows) % N_USERS
    rng = np.random.default_rng(11)
    seen = [np.array([b % N_ITEMS]) for b in range(n_rows)]
    targets = [rng.integers(0, N_ITEMS, 1 + b % 4) for b in range(n_rows)]
    targets[-1] = np.arange(N_ITEMS - MAX_T, N_ITEMS)               # the last tiles of the last slice, for the last row
    dev = _Device(*_host(f, "exact"), f, ld, bias, users)
    want = _want_exact(M, users, seen, targets, N_ITEMS)
    _check_exact(dev.positions(n_rows, N_ITEMS, n_slices, targets, seen), want, "scan cap")
    assert want[0][-MAX_T:].max() > 100


def test_rank_positions_beyond_the_row_grid_cap():
    """More rows than the target and finish kernels' workgroups take in one trip (four each)."""
    f, bias = 5, 1
    n_rows = 4 * _constant("WMF_RANKPOS_ROW_GRID", "recmodel_amd/csrc/wmf_rankpos.hip") + 37
    ld = _ld(f)
    M, _ = _scores(f, bias, "exact")
    users = np.arange(n_rows) % N_USERS
    seen = [np.sort(np.array([b % N_ITEMS, (7 * b) % N_ITEMS])) if b % 2 else np.arange(0) for b in range(n_rows)]
    targets = [np.array([(3 * b) % N_ITEMS, b % N_ITEMS]) for b in range(n_rows)]
    dev = _Device(*_host(f, "exact"), f, ld, bias, users)
    want = _want_exact(M, users, seen, targets, N_ITEMS)
    for n_slices in (1, 2):
        _check_exact(dev.positions(n_rows, N_ITEMS, n_slices, targets, seen), want, ("row cap", n_slices))
    assert (want[0] == pref.SEEN).sum() > 100
