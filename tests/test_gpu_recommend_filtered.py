"""wmf_recommend_topn_filtered and wmf_similar_topn_filtered through the C ABI, per element: the fused top-n over a PART of the
catalogue, given as allow masks (tested where an item would be inserted) or as a list of candidate rows (only those are scored).

The reference is tests/recommend_ref.py with the ineligible items added to the row's seen list (tests/filter_cases.py).  A score
does not depend on the tile position an item has, so every comparison is exact: the EXACT class against the reference, both classes
bit for bit against the unfiltered entry points given the complement as seen items.  Only the order of the ROUNDED class is held to
the bound B of tests/serving_ref.py, through _check_rounded_order on the eligible unseen items."""
import numpy as np
import pytest
import torch

import filter_cases as fc
import recommend_ref as rref
import serving_ref as ref
from scan_cases import N_ITEMS, N_USERS, _api, _check_rounded_order, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list, case
from test_gpu_recommend import _Recommend

pytestmark = pytest.mark.gpu

TOPNS = (1, 10, 128)
SLICES = (1, 2, 3, 7, 19, 256)
WIDE = [(f, b) for f in (5, 64, 129, 260) for b in (0, 1)]
wide = pytest.mark.parametrize("f,bias", WIDE)
EVERYTHING = np.arange(N_ITEMS)


def _with_complement(seen, masks):
    """The seen rows with the ineligible items of each row's mask added, ascending."""
    return [np.sort(np.concatenate([np.asarray(s, dtype=np.int64), np.flatnonzero(~m)])) for s, m in zip(seen, masks)]


def _check_exact(got, M, users, seen, masks, topn, what):
    items, sc, cnt = got
    want = [fc.filtered_ref(M[u], seen[b], masks[b], topn) for b, u in enumerate(users)]
    want_items = rref.padded_rows(want, topn, -1, np.int32)
    assert np.array_equal(items, want_items), (what, np.argwhere(items != want_items)[:5])
    assert np.array_equal(cnt, [len(w) for w in want]), what
    valid = want_items >= 0
    assert (sc[~valid] == -np.inf).all(), what
    assert np.array_equal(sc[valid].astype(np.int64), M[np.repeat(users, valid.sum(axis=1)), want_items[valid]]), what
    assert np.array_equal(sc[valid], np.rint(sc[valid])), what


# --------------------------------------------------------------------------------------------- 1. the mask form, both classes
@case
def test_mask_form_exact(f, bias, extra):
    """Every pattern x topn at every width: items, scores and counts equal the reference; padding -1 / -inf; sentinels intact."""
    ld = _ld(f, extra)
    M, _ = _scores(f, bias, "exact")
    for pattern in range(len(fc.PATTERNS)):
        users, seen, masks = fc.case_rows(f, bias, "exact", pattern)
        run = fc.Filtered(*_host(f, "exact"), f, ld, bias, users)
        bits, allow_idx = fc.bits_of(pattern, masks)
        for topn in TOPNS:
            got = run(topn, 0, seen, bits=bits, allow_idx=allow_idx)
            _check_exact(got, M, users, seen, masks, topn, (f, bias, ld, fc.PATTERNS[pattern], topn))


@case
def test_mask_form_rounded(f, bias, extra):
    """The ROUNDED class: eligible, unique, counts and padding exact; scores within B, best first; the order within B."""
    ld = _ld(f, extra)
    R, B = _scores(f, bias, "rounded")
    for pattern in range(len(fc.PATTERNS)):
        users, seen, masks = fc.case_rows(f, bias, "rounded", pattern)
        run = fc.Filtered(*_host(f, "rounded"), f, ld, bias, users)
        bits, allow_idx = fc.bits_of(pattern, masks)
        topn = TOPNS[pattern % len(TOPNS)]
        items, sc, cnt = run(topn, 0, seen, bits=bits, allow_idx=allow_idx)
        for b, u in enumerate(users):
            what = (f, bias, ld, fc.PATTERNS[pattern], topn, b)
            elig = np.setdiff1d(np.flatnonzero(masks[b]), seen[b])
            k = min(topn, len(elig))
            assert cnt[b] == k and (items[b, k:] == -1).all() and (sc[b, k:] == -np.inf).all(), what
            if k == 0:
                continue
            it = items[b, :k].astype(np.int64)
            assert np.isin(it, elig).all() and len(np.unique(it)) == k, what
            assert (np.abs(sc[b, :k].astype(np.float64) - R[u, it]) <= B[u, it]).all() and (np.diff(sc[b, :k]) <= 0).all(), what
            _check_rounded_order(np.searchsorted(elig, it), R[u, elig], B[u, elig], what)


# ------------------------------------------------------------------------------- 2. bit for bit against the existing entry
@wide
@pytest.mark.parametrize("cls", ("exact", "rounded"))
def test_mask_form_is_the_existing_entry_with_the_complement_seen(f, bias, cls):
    ld = _ld(f)
    for pattern in (8, 9, 6, 11):
        users, seen, masks = fc.case_rows(f, bias, cls, pattern)
        run, old = fc.Filtered(*_host(f, cls), f, ld, bias, users), _Recommend(*_host(f, cls), f, ld, bias, users)
        bits, allow_idx = fc.bits_of(pattern, masks)
        for topn in (10, 128):
            want = old(N_USERS, N_ITEMS, topn, 0, _with_complement(seen, masks))
            assert fc.same_bits(run(topn, 0, seen, bits=bits, allow_idx=allow_idx), want), (f, bias, cls, pattern, topn)
            assert fc.same_bits(run(topn, 0, seen, bits=bits, allow_idx=allow_idx), want), "two runs, the same bits"


# ------------------------------------------------------------------------------------------------------- 3. per-row masks
@wide
def test_per_row_masks(f, bias):
    """Four masks, allow_idx cycling -1, 0, 1, 2, 3: user 2 stands at positions 2 and 9 under masks 1 and 3.  Each row is the
    single-mask call's row; the -1 rows are the unfiltered entry's."""
    ld = _ld(f)
    users = _user_list()
    assert users[2] == users[9]
    M, _ = _scores(f, bias, "exact")
    rng = np.random.default_rng(40 + f)
    seen = _seen_rows(rng, M[users], N_ITEMS, 3)
    G = np.stack([fc.mask_row(p, rng, M[0], [], N_ITEMS) for p in (9, 6, 5, 7)])
    allow_idx = np.arange(N_USERS) % 5 - 1
    assert allow_idx[2] == 1 and allow_idx[9] == 3
    run, old = fc.Filtered(*_host(f, "exact"), f, ld, bias, users), _Recommend(*_host(f, "exact"), f, ld, bias, users)
    got = run(10, 0, seen, bits=fc.pack(G), allow_idx=allow_idx)
    single = [run(10, 0, seen, bits=fc.pack(G[g])) for g in range(4)] + [old(N_USERS, N_ITEMS, 10, 0, seen)]
    for b in range(N_USERS):
        assert fc.same_bits([a[b] for a in got], [a[b] for a in single[allow_idx[b]]]), (f, bias, b)
    masks = np.where(allow_idx[:, None] < 0, True, G[allow_idx])
    _check_exact(got, M, users, seen, masks, 10, (f, bias, "per-row masks"))
    assert not np.array_equal(got[0][2], got[0][9])


# ------------------------------------------------------------------------------------------------------- 4. the list form
def _lists(rng):
    out = [np.array([137]), np.array([0]), np.array([N_ITEMS - 1])]
    for n in (15, 16, 17, 33):
        ids = np.sort(rng.choice(N_ITEMS, n, replace=False))
        ids[0], ids[-1] = 0, N_ITEMS - 1                            # the first and the last item of the catalogue
        out.append(ids)
    return out + [np.sort(rng.choice(np.arange(1, N_ITEMS - 1), 33, replace=False)), EVERYTHING]


@wide
def test_list_form(f, bias):
    """Lists of 1, 15, 16, 17, 33 and 300 ids, with and without seen rows, topn beyond the list: the reference in the EXACT class,
    and in both classes the bits of the mask form with the list's indicator mask.  All 300 ids: the unfiltered entry."""
    ld = _ld(f)
    users = _user_list()
    rng = np.random.default_rng(50 + f + bias)
    for cls in ("exact", "rounded"):
        S, _ = _scores(f, bias, cls)
        seen_rows = _seen_rows(rng, S[users], N_ITEMS, 5)
        run, old = fc.Filtered(*_host(f, cls), f, ld, bias, users), _Recommend(*_host(f, cls), f, ld, bias, users)
        for cand in _lists(rng):
            mask = np.isin(EVERYTHING, cand)
            for seen in (seen_rows, None):
                for topn in (10, 128) if len(cand) in (17, 300) else (10,):
                    what = (f, bias, cls, len(cand), seen is not None, topn)
                    got = run(topn, 0, seen, cand=cand)
                    assert fc.same_bits(got, run(topn, 0, seen, bits=fc.pack(mask))), what
                    if cls == "exact":
                        _check_exact(got, S, users, seen or [[]] * N_USERS, np.tile(mask, (N_USERS, 1)), topn, what)
                    if len(cand) == N_ITEMS:
                        assert fc.same_bits(got, old(N_USERS, N_ITEMS, topn, 0, seen)), what
                    if len(cand) < topn and seen is None:
                        assert (got[2] == len(cand)).all()


# ------------------------------------------------------------------------------------------------------------ 5. slices
@pytest.mark.parametrize("f,bias", [(5, 1), (129, 0)])
def test_the_result_does_not_depend_on_the_slices(f, bias):
    ld = _ld(f)
    M, _ = _scores(f, bias, "exact")
    users, seen, masks = fc.case_rows(f, bias, "exact", 9)
    run = fc.Filtered(*_host(f, "exact"), f, ld, bias, users)
    bits, allow_idx = fc.bits_of(9, masks)
    cand = np.flatnonzero(masks[0])
    assert len(cand) > 64
    for topn in (10, 128):
        first_mask, first_list = run(topn, 0, seen, bits=bits, allow_idx=allow_idx), run(topn, 0, seen, cand=cand)
        _check_exact(first_mask, M, users, seen, masks, topn, (f, bias, topn))
        _check_exact(first_list, M, users, seen, np.tile(masks[0], (N_USERS, 1)), topn, (f, bias, topn, "list"))
        for n_slices in SLICES:
            assert fc.same_bits(run(topn, n_slices, seen, bits=bits, allow_idx=allow_idx), first_mask), (f, bias, topn, n_slices)
            assert fc.same_bits(run(topn, n_slices, seen, cand=cand), first_list), (f, bias, topn, n_slices, "list")


# ----------------------------------------------------------------------------------- 6. the grid cap and the wave-count switch
def test_mask_form_beyond_the_scan_grid_cap():
    """More (user block, slice) pairs than workgroups, as test_recommend_beyond_the_scan_grid_cap, under a mask."""
    f, bias, topn, n_slices = 5, 1, 10, 256
    cap = _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    n_users = 64 * (cap // n_slices) + 1
    assert ((n_users + 63) // 64) * n_slices > cap >= (n_users // 64) * n_slices
    M, _ = _scores(f, bias, "exact")
    users = np.arange(n_users) % N_USERS
    seen = [np.array([b % N_ITEMS]) for b in range(n_users)]
    mask = fc.mask_row(6, None, None, None, N_ITEMS)
    run = fc.Filtered(*_host(f, "exact"), f, _ld(f), bias, users)
    _check_exact(run(topn, n_slices, seen, bits=fc.pack(mask)), M, users, seen, np.tile(mask, (n_users, 1)), topn, "scan cap, mask")
    _check_exact(run(topn, n_slices, seen, cand=np.flatnonzero(mask)), M, users, seen, np.tile(mask, (n_users, 1)), topn, "scan cap, list")


@pytest.mark.parametrize("f,bias", [(64, 0), (129, 1), (260, 1)])
def test_both_sides_of_the_wave_count_switch(f, bias):
    """topn = 64: four waves; topn = 65: two.  65 batch positions, 257 items, both forms."""
    nu, ni = 65, 257
    M, _ = _scores(f, bias, "exact")
    users = _user_list(nu)
    rng = np.random.default_rng(3100 + 2 * f + bias)
    seen = _seen_rows(rng, M[users], ni, 0)
    mask = fc.mask_row(5, rng, None, None, ni)
    Uf, If = _host(f, "exact")
    run = fc.Filtered(Uf, If[:ni], f, _ld(f), bias, users)
    for topn in (64, 65):
        got = run(topn, 0, seen, bits=fc.pack(mask))
        _check_exact(got, M[:, :ni], users, seen, np.tile(mask, (nu, 1)), topn, (f, bias, topn))
        assert fc.same_bits(run(topn, 3, seen, cand=np.flatnonzero(mask)), got), (f, bias, topn)
        assert (got[2] == topn).any() and (got[2] < topn).any()


# --------------------------------------------------------------------------------------------------------------- 7. ties
@pytest.mark.parametrize("f,bias", [(5, 0), (5, 1), (129, 0)])
def test_ties_go_to_the_lower_eligible_id(f, bias):
    """All-zero user rows: every score ties (or is the item's bias); the answer is the first eligible ids, in both forms."""
    Uf, If = _host(f, "exact")
    zero = np.flatnonzero((Uf == 0).all(axis=1))
    assert len(zero) >= 5
    M, _ = _scores(f, bias, "exact")
    users = np.resize(zero, 20)
    rng = np.random.default_rng(f)
    seen = [np.sort(rng.choice(N_ITEMS, 40, replace=False)) if b % 2 else np.arange(b) for b in range(20)]
    mask = fc.mask_row(6, None, None, None, N_ITEMS)
    mask[1:40:4] = True
    run = fc.Filtered(Uf, If, f, _ld(f), bias, users)
    for topn in (10, 128):
        for n_slices in (0, 3):
            got = run(topn, n_slices, seen, bits=fc.pack(mask))
            _check_exact(got, M, users, seen, np.tile(mask, (20, 1)), topn, (f, bias, topn, n_slices))
            assert fc.same_bits(run(topn, n_slices, seen, cand=np.flatnonzero(mask)), got)
            if not bias:
                for b in range(20):
                    assert np.array_equal(got[0][b], np.setdiff1d(np.flatnonzero(mask), seen[b])[:topn]), (f, topn, b)


# ------------------------------------------------------------------------------------------- 8. wmf_similar_topn_filtered
def _similar(filtered, Cd, f, ld, bias, norms, query_idx, exclude_self, excl, topn, bits=None, allow_idx=None):
    _lib, lib, _ptr, _stream = _api()
    nq = len(query_idx)
    ws = torch.empty(int(lib.wmf_similar_workspace_bytes(nq, topn, 0)), dtype=torch.uint8, device="cuda")
    rows = torch.full((nq + 1, topn), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((nq + 1, topn), fc.SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.full((nq + 1,), -7, dtype=torch.int32, device="cuda")
    ip_d = idx_d = None
    if excl is not None:
        indptr, indices = rref.csr_of(excl)
        ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
    q_d = _dev(query_idx, np.int32)                                 # (every device array is held until the outputs are read)
    head = (_ptr(Cd), _ptr(Cd), f, ld, bias, _ptr(norms), _ptr(norms), _ptr(q_d), nq, N_ITEMS, int(exclude_self), _ptr(ip_d), _ptr(idx_d))
    tail = (topn, 0, _ptr(rows), _ptr(sc), _ptr(cnt), _ptr(ws), ws.numel(), _stream())
    if filtered:
        bits_d = None if bits is None else _dev(np.atleast_2d(bits).view(np.int32))
        ai_d = None if allow_idx is None else _dev(allow_idx, np.int32)
        shape = (0, 0) if bits is None else np.atleast_2d(bits).shape
        _lib.check(lib.wmf_similar_topn_filtered(*head, _ptr(bits_d), shape[1], shape[0], _ptr(ai_d), *tail))
    else:
        _lib.check(lib.wmf_similar_topn(*head, *tail))
    rows, sc, cnt = rows.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
    del q_d
    assert (rows[-1] == -7).all() and (sc[-1] == np.float32(fc.SENTINEL)).all() and cnt[-1] == -7
    return rows[:-1], sc[:-1], cnt[:-1]


@wide
@pytest.mark.parametrize("cosine", (False, True))
def test_similar_filtered_is_similar_with_the_complement_excluded(f, bias, cosine):
    _lib, lib, _ptr, _stream = _api()
    ld = _ld(f)
    rng = np.random.default_rng(60 + f + bias)
    queries = np.array([0, N_ITEMS - 1, 2, 15, 16, 17, 31, 32, 33, 2] + [(37 * b + 5) % N_ITEMS for b in range(10, N_USERS)])
    for cls in ("exact", "rounded"):
        Cd = _dev(ref.padded(_host(f, cls)[1], ld))
        norms = None
        if cosine:
            norms = torch.empty(N_ITEMS, dtype=torch.float32, device="cuda")
            _lib.check(lib.wmf_row_inv_norms(_ptr(Cd), N_ITEMS, f, ld, bias, _ptr(norms), _stream()))
        G = np.stack([fc.mask_row(p, rng, None, None, N_ITEMS) for p in (9, 6, 4, 7)])
        G[:, queries[:20]] = True                                   # the own id is allowed: exclude_self still removes it
        allow_idx = np.arange(N_USERS) % 5 - 1
        masks = np.where(allow_idx[:, None] < 0, True, G[allow_idx])
        complement = [np.flatnonzero(~m) for m in masks]
        for exclude_self in (True, False):
            want = _similar(False, Cd, f, ld, bias, norms, queries, exclude_self, complement, 10)
            got = _similar(True, Cd, f, ld, bias, norms, queries, exclude_self, None, 10, fc.pack(G), allow_idx)
            assert fc.same_bits(got, want), (f, bias, cosine, cls, exclude_self)
            own = (got[0] == queries[:, None]).any(axis=1)
            assert not own.any() if exclude_self else own.any()
        one = _similar(True, Cd, f, ld, bias, norms, queries, True, None, 10, fc.pack(G[0]))
        assert fc.same_bits(one, _similar(False, Cd, f, ld, bias, norms, queries, True, [np.flatnonzero(~G[0])] * N_USERS, 10))
        assert fc.same_bits(_similar(True, Cd, f, ld, bias, norms, queries, True, None, 10), _similar(False, Cd, f, ld, bias, norms, queries, True, None, 10))


# ----------------------------------------------------------------------------------------------------- 9. which kernel ran
def _launched(run):
    _lib, lib, _ptr, _stream = _api()
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        lib.wmf_profile_enable(0)
    names = {name for name, *_ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return names


def test_a_filtered_call_runs_a_filtered_kernel_and_an_unfiltered_one_the_old_kernels():
    f, bias = 5, 1
    ld = _ld(f)
    users = _user_list()
    run, old = fc.Filtered(*_host(f, "exact"), f, ld, bias, users), _Recommend(*_host(f, "exact"), f, ld, bias, users)
    mask = fc.mask_row(6, None, None, None, N_ITEMS)
    plain = {"recommend_scan_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: old(N_USERS, N_ITEMS, 10, 0)) == plain
    assert _launched(lambda: run(10, 0)) == plain                   # neither form: wmf_recommend_topn
    assert _launched(lambda: run(10, 0, bits=fc.pack(mask))) == {"recommend_scan_mask_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: run(65, 0, bits=fc.pack(mask))) == {"recommend_scan_mask_kernel<4, 4, 2>", "recommend_merge_kernel"}
    assert _launched(lambda: run(10, 0, cand=np.flatnonzero(mask))) == {"recommend_scan_list_kernel<4, 4, 4>", "recommend_merge_kernel"}
    Cd = _dev(ref.padded(_host(f, "exact")[1], ld))
    q = np.arange(N_USERS)
    assert _launched(lambda: _similar(True, Cd, f, ld, bias, None, q, True, None, 10, fc.pack(mask))) == {"similar_scan_mask_kernel<4, 4, 4>", "recommend_merge_kernel"}
    same = {"similar_scan_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: _similar(True, Cd, f, ld, bias, None, q, True, None, 10)) == same
    assert _launched(lambda: _similar(False, Cd, f, ld, bias, None, q, True, None, 10)) == same
    assert fc.same_bits(run(10, 0), old(N_USERS, N_ITEMS, 10, 0))


# -------------------------------------------------------------------------------------------------------- 10. WMF_EINVAL
def test_refusals_come_before_any_launch():
    _lib = _api()[0]
    f, bias = 5, 1
    run = fc.Filtered(*_host(f, "exact"), f, _ld(f), bias, _user_list())
    bits, cand = fc.pack(fc.mask_row(6, None, None, None, N_ITEMS)), np.arange(0, N_ITEMS, 3)
    assert bits.shape == (1, 10)

    def refused():
        run(10, 0, bits=bits, cand=cand, expect=_lib.WMF_EINVAL)                  # both forms in one call
        run(10, 0, bits=bits, n_masks=0, expect=_lib.WMF_EINVAL)
        run(10, 0, bits=bits, allow_words=9, expect=_lib.WMF_EINVAL)              # 300 items need 10 words
        run(10, 0, cand=cand, n_cand=0, expect=_lib.WMF_EINVAL)
        run(10, 0, bits=bits, ws_bytes=255, expect=_lib.WMF_EINVAL)
        run(10, 0, cand=cand, ws_bytes=255, expect=_lib.WMF_EINVAL)
    assert _launched(refused) == set()
