"""wmf_recommend_topn through the C ABI, per element (csrc/wmf_recommend.hip): the N best items of the whole catalogue for a batch
of users, each user's seen items left out, by one fused scan (f32 MFMA scores, a running top-n per user in LDS, the catalogue
cut into slices that a second kernel merges).

The vocabulary of tests/test_gpu_serving.py: the same widths, bias settings and leading dimensions, the same two input classes
(tests/serving_ref.py) -- EXACT, integers, where the device must equal tests/recommend_ref.py bit for bit and equal scores are
real ties, and ROUNDED, standard normal, held to the derived bound B(u, i).  Shapes are the smallest at which the kernel can go
wrong: user counts around the 16 users of a wave, catalogue lengths around the 16-item tile and the stage, every slice count from
one to more slices than tiles, topn from 1 to the maximum and beyond the catalogue.  The result may not depend on the slices."""
import numpy as np
import pytest
import torch

import recommend_ref as rref
import serving_ref as ref
from conftest import record_error
from scan_cases import N_ITEMS, N_PATTERNS, N_USERS, _api, _check_rounded_order, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list, case

pytestmark = pytest.mark.gpu

GRID_USERS, GRID_ITEMS, GRID_TOPN, GRID_SLICES = (1, 15, 16, 17, 33, 40), (1, 15, 16, 17, 255, 256, 257, 300), (1, 2, 10, 64, 128), (0, 1, 2, 3, 7, 64)
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------------------------------ helpers
class _Recommend:
    """wmf_recommend_topn on prefixes of one user list and of one item matrix."""

    def __init__(self, Uf, If, f, ld, bias, user_idx):
        self.Ud, self.Id, self.args = _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld)), (f, ld, bias)
        self.user_idx = _dev(user_idx, np.int32)

    def __call__(self, n_users, n_items, topn, n_slices, seen=None, scores=True, count=True):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        ws = torch.empty(int(lib.wmf_recommend_workspace_bytes(n_users, topn, n_slices)), dtype=torch.uint8, device="cuda")
        items = torch.full((n_users, topn), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((n_users, topn), SENTINEL, dtype=torch.float32, device="cuda") if scores else None
        cnt = torch.full((n_users,), -7, dtype=torch.int32, device="cuda") if count else None
        ip_d = idx_d = None
        if seen is not None:
            indptr, indices = rref.csr_of(seen)
            assert len(indptr) == n_users + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        _lib.check(lib.wmf_recommend_topn(_ptr(self.Ud), _ptr(self.Id), f, ld, bias, _ptr(self.user_idx), n_users, n_items, _ptr(ip_d),
                                          _ptr(idx_d), topn, n_slices, _ptr(items), _ptr(sc), _ptr(cnt), _ptr(ws), ws.numel(), _stream()))
        return items.cpu().numpy(), (sc.cpu().numpy() if scores else None), (cnt.cpu().numpy() if count else None)


def _check_exact(got, M, users, seen, n_items, topn, what):
    items, sc, cnt = got
    want = [rref.recommend_ref(M[u, :n_items], [] if seen is None else seen[b], topn) for b, u in enumerate(users)]
    want_items = rref.padded_rows(want, topn, -1, np.int32)
    assert np.array_equal(items, want_items), (what, np.argwhere(items != want_items)[:5])
    assert np.array_equal(cnt, [len(w) for w in want]), what
    valid = want_items >= 0
    assert (sc[~valid] == -np.inf).all() and np.array_equal(sc[valid].astype(np.int64), M[np.repeat(users, valid.sum(axis=1)), want_items[valid]]), what
    assert np.array_equal(sc[valid], np.rint(sc[valid])), what


# ------------------------------------------------------------------------------------------- 1. the grid, both input classes
@case
def test_recommend_topn(f, bias, extra):
    ld = _ld(f, extra)
    rng = np.random.default_rng(1000 + 2 * f + bias)
    users = _user_list()
    patterns, null_rows, short = set(), 0, 0
    # EXACT: bit for bit, every slice count the same answer
    M, _ = _scores(f, bias, "exact")
    rec = _Recommend(*_host(f, "exact"), f, ld, bias, users)
    for iu, nu in enumerate(GRID_USERS):
        for ii, ni in enumerate(GRID_ITEMS):
            seen = _seen_rows(rng, M[users[:nu]], ni, iu + ii)
            patterns |= {(b + iu + ii) % N_PATTERNS for b in range(nu)}
            for topn in GRID_TOPN:
                first = None
                for n_slices in GRID_SLICES:
                    got = rec(nu, ni, topn, n_slices, seen)
                    if first is None:
                        first = got
                        _check_exact(got, M, users[:nu], seen, ni, topn, (f, bias, ld, nu, ni, topn, n_slices))
                        short += int((got[2] < topn).sum())
                    else:
                        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, first)), (f, bias, ld, nu, ni, topn, n_slices)
            if nu == N_USERS:                                       # seen_indptr = NULL, and once without scores and counts
                topn = GRID_TOPN[ii % len(GRID_TOPN)]
                got = rec(nu, ni, topn, GRID_SLICES[ii % len(GRID_SLICES)], None)
                _check_exact(got, M, users[:nu], None, ni, topn, (f, bias, ld, nu, ni, topn, "no seen list"))
                assert np.array_equal(rec(nu, ni, topn, 2, None, scores=False, count=False)[0], got[0])
                null_rows += nu
    assert patterns == set(range(N_PATTERNS)) and null_rows and short
    # ROUNDED: eligible, unique, scores within B, best first by the device's own scores, the order within B
    R, B = _scores(f, bias, "rounded")
    rec = _Recommend(*_host(f, "rounded"), f, ld, bias, users)
    worst_score = worst_order = 0.0
    for ii, ni in enumerate(GRID_ITEMS):
        topn = GRID_TOPN[ii % len(GRID_TOPN)]
        seen = _seen_rows(rng, R[users], ni, ii)
        first = None
        for n_slices in (0, 3):
            what = (f, bias, ld, ni, topn, n_slices)
            items, sc, cnt = got = rec(N_USERS, ni, topn, n_slices, seen)
            if first is not None:
                assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, first)), what
                continue
            first = got
            for b, u in enumerate(users):
                elig = np.setdiff1d(np.arange(ni), seen[b])
                k = min(topn, len(elig))
                assert cnt[b] == k and (items[b, k:] == -1).all() and (sc[b, k:] == -np.inf).all(), (what, b)
                if k == 0:
                    continue
                it = items[b, :k].astype(np.int64)
                assert np.isin(it, elig).all() and len(np.unique(it)) == k, (what, b)
                worst_score = max(worst_score, float((np.abs(sc[b, :k].astype(np.float64) - R[u, it]) / B[u, it]).max()))
                assert (np.diff(sc[b, :k]) <= 0).all(), (what, b)
                worst_order = max(worst_order, _check_rounded_order(np.searchsorted(elig, it), R[u, elig], B[u, elig], (what, b)))
    assert worst_score <= 1.0, (f, bias, ld, worst_score)
    record_error("serving_recommend_scan_kernel", **{f"f{f}_bias{bias}_ld{ld}": worst_score})
    record_error("serving_recommend_order", **{f"f{f}_bias{bias}_ld{ld}": worst_order})


# ------------------------------------------------------------------------------------------------------- 2. tie pressure
@pytest.mark.parametrize("f,bias", [(1, 0), (5, 0), (5, 1), (129, 0), (129, 1)])
def test_recommend_ties_go_to_the_lower_item_id(f, bias):
    """All-zero user rows of the EXACT class: every score ties (or equals the item's bias), so the answer is the first topn
    eligible ids (by bias, then id) -- at every slice count, with ties across tile and slice boundaries."""
    ld = _ld(f)
    Uf, If = _host(f, "exact")
    zero = np.flatnonzero((Uf == 0).all(axis=1))
    assert len(zero) >= 5
    M, _ = _scores(f, bias, "exact")
    users = np.resize(zero, 20)
    rng = np.random.default_rng(f)
    seen = [np.sort(rng.choice(N_ITEMS, 40, replace=False)) if b % 2 else np.arange(b) for b in range(20)]
    rec = _Recommend(Uf, If, f, ld, bias, users)
    if not bias:
        assert (M[zero] == 0).all()                                  # a tie group of 300 at every place
    for topn in (10, 128):
        for n_slices in GRID_SLICES:
            got = rec(20, N_ITEMS, topn, n_slices, seen)
            _check_exact(got, M, users, seen, N_ITEMS, topn, (f, bias, topn, n_slices))
            if not bias:
                for b in range(20):
                    assert np.array_equal(got[0][b], np.setdiff1d(np.arange(N_ITEMS), seen[b])[:topn]), (f, topn, n_slices, b)


# -------------------------------------------------------------------------------------------------- 3. threshold pressure
def _pressure_values(n):
    i = np.arange(n)
    mix = np.where(i % 3 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert np.signbit(mix).sum() > n // 4
    return {"ascending": i.astype(np.float32), "descending": (n - i).astype(np.float32), "constant": np.full(n, 2.5, dtype=np.float32),
            "sawtooth": (i % 37).astype(np.float32) - 18, "signed zeros": mix}


@pytest.mark.parametrize("shape", ("ascending", "descending", "constant", "sawtooth", "signed zeros"))
def test_recommend_under_threshold_pressure(shape):
    """f = 1 and a user factor of 1.0: score = item value, exact in float32.  Ascending values beat the threshold with every
    item, so the buffer is cut back again and again; constant values and signed zeros tie throughout."""
    n = 5000
    values = _pressure_values(n)[shape]
    rec = _Recommend(np.ones((2, 1), dtype=np.float32), values[:, None], 1, _ld(1), 0, [0, 1])
    seen = [np.arange(0), np.arange(n - 40, n - 5)]
    for topn in (1, 10, 128):
        want = [rref.recommend_ref(values.astype(np.float64), s, topn) for s in seen]
        for n_slices in (1, 3):
            items, sc, cnt = rec(2, n, topn, n_slices, seen)
            assert np.array_equal(items, np.stack(want)), (shape, topn, n_slices)
            assert np.array_equal(sc.view(np.uint32), (values[np.stack(want)] + np.float32(0.0)).view(np.uint32)), (shape, topn, n_slices)
            assert cnt.tolist() == [topn, topn]


# -------------------------------------------------------------------------------------- 4. agreement with the existing path
@case
def test_recommend_agrees_with_rank_topn_batch(f, bias, extra):
    """No exclusions: positions and scores of wmf_rank_topn_batch over cand = arange(n_items) -- the same MFMA arithmetic, so
    bit for bit in both input classes."""
    _lib, lib, _ptr, _stream = _api()
    ld = _ld(f, extra)
    users = _user_list()
    cand = _dev(np.arange(N_ITEMS), np.int32)
    ws = torch.empty(int(lib.wmf_rank_batch_workspace_bytes(N_USERS, N_ITEMS)), dtype=torch.uint8, device="cuda")
    for cls in ("exact", "rounded"):
        rec = _Recommend(*_host(f, cls), f, ld, bias, users)
        for topn, n_slices in ((10, 0), (128, 3)):
            pos = torch.full((N_USERS, topn), -1, dtype=torch.int32, device="cuda")
            sc = torch.full((N_USERS, topn), SENTINEL, dtype=torch.float32, device="cuda")
            _lib.check(lib.wmf_rank_topn_batch(_ptr(rec.Ud), _ptr(rec.Id), f, ld, bias, _ptr(rec.user_idx), N_USERS, _ptr(cand), N_ITEMS,
                                               topn, _ptr(pos), _ptr(sc), _ptr(ws), ws.numel(), _stream()))
            items, scores, cnt = rec(N_USERS, N_ITEMS, topn, n_slices)
            assert np.array_equal(items, pos.cpu().numpy()), (f, bias, ld, cls, topn)
            assert np.array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32)), (f, bias, ld, cls, topn)
            assert (cnt == topn).all()


# ------------------------------------------------------------------------------------------------- 5. the wave-count switch
@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("f", (64, 129, 260))
def test_recommend_on_both_sides_of_the_wave_count_switch(f, bias):
    """topn = 64 is the last of the four-wave workgroup (64 batch positions), topn = 65 the first of the two-wave one (32), each
    its own instantiation of the scan.  65 batch positions are two blocks of the first and three of the second, the last one
    partial either way; 257 items end in a one-item tile.  EXACT class: bit for bit at the first slice count, the other slice
    counts the same bits, and the 64 best of the topn = 65 answer are the topn = 64 answer."""
    nu, ni = 65, 257
    ld = _ld(f)
    M, _ = _scores(f, bias, "exact")
    users = _user_list(nu)
    seen = _seen_rows(np.random.default_rng(3000 + 2 * f + bias), M[users], ni, 0)
    rec = _Recommend(*_host(f, "exact"), f, ld, bias, users)
    answers = {}
    for topn in (64, 65):
        for n_slices in (0, 1, 3):
            got = rec(nu, ni, topn, n_slices, seen)
            if topn not in answers:
                answers[topn] = got
                _check_exact(got, M, users, seen, ni, topn, (f, bias, ld, topn, n_slices))
            else:
                assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, answers[topn])), (f, bias, ld, topn, n_slices)
    (items64, sc64, cnt64), (items65, sc65, cnt65) = answers[64], answers[65]
    assert np.array_equal(items65[:, :64], items64) and np.array_equal(sc65[:, :64].view(np.int32), sc64.view(np.int32))
    assert np.array_equal(np.minimum(cnt65, 64), cnt64) and (cnt65 == 65).any() and (cnt64 < 64).any()


# ------------------------------------------------------------------------------------------------------ 6. grid-stride caps
def test_recommend_beyond_the_scan_grid_cap():
    """More (user block, slice) pairs than workgroups: 17 blocks of 64 users x the largest slice count.  Then the best items of
    the last block's user in the last tile, which the second trip scans."""
    f, bias, topn = 5, 1, 10
    n_slices = 256
    cap = _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    n_users = 64 * (cap // n_slices) + 1
    assert ((n_users + 63) // 64) * n_slices > cap >= (n_users // 64) * n_slices
    ld = _ld(f)
    Uf, If = _host(f, "exact")
    M, _ = _scores(f, bias, "exact")
    users = np.arange(n_users) % N_USERS
    seen = [np.array([b % N_ITEMS]) for b in range(n_users)]
    got = _Recommend(Uf, If, f, ld, bias, users)(n_users, N_ITEMS, topn, n_slices, seen)
    _check_exact(got, M, users, seen, N_ITEMS, topn, "scan cap")
    last = users[-1]
    order = np.argsort(-M[last], kind="stable")
    I2 = np.repeat(If[order[-1:]], N_ITEMS, axis=0)
    I2[288:] = If[order[:12]]
    M2 = ref.score_matrix_int(Uf, I2, np.arange(N_USERS), np.arange(N_ITEMS), bias)
    got = _Recommend(Uf, I2, f, ld, bias, users)(n_users, N_ITEMS, topn, n_slices, seen)
    _check_exact(got, M2, users, seen, N_ITEMS, topn, "scan cap, late winners")
    assert (got[0][-1] >= 288).all() and M2[last, 288] > M2[last, 0]


def test_recommend_beyond_the_merge_grid_cap():
    """More users than the merge kernel's workgroups take in one trip (four each)."""
    f, bias, topn = 5, 1, 10
    n_users = 4 * _constant("WMF_REC_MERGE_GRID", "recmodel_amd/csrc/wmf_recommend.hip") + 37
    ld = _ld(f)
    M, _ = _scores(f, bias, "exact")
    users = np.arange(n_users) % N_USERS
    seen = [np.array([b % N_ITEMS, (7 * b) % N_ITEMS]) if b % 2 else np.arange(0) for b in range(n_users)]
    seen = [np.sort(s) for s in seen]
    rec = _Recommend(*_host(f, "exact"), f, ld, bias, users)
    for n_slices in (1, 2):
        _check_exact(rec(n_users, N_ITEMS, topn, n_slices, seen), M, users, seen, N_ITEMS, topn, ("merge cap", n_slices))
