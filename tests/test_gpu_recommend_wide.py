"""wmf_recommend_topn_wide through the C ABI, per element: the fused top-n for 1 <= topn <= 4096, the running keys of a row in the
workspace instead of LDS, cut back by an exact radix select, and a selection kernel that sorts the topn best of a row's slices.

The reference is tests/recommend_ref.py and serving_ref.stable_topn on the host, the ineligible items of a filter added to the seen
rows (tests/filter_cases.py).  Every comparison is for equality: the EXACT class against the int64 reference, both classes bit for
bit against the kernels of wmf_recommend_topn[_filtered] for topn <= 128, and the ROUNDED class at topn 1000 against the host top-n
of the device's own float32 scores (wmf_rank_topn_batch: the same arithmetic).  Every call keeps a guard region past its workspace and
a sentinel row on either side of its outputs."""
import functools

import numpy as np
import pytest
import torch

import filter_cases as fc
import recommend_ref as rref
import serving_ref as ref
from scan_cases import N_ITEMS, N_USERS, _api, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list, case
from test_gpu_recommend import _Recommend

pytestmark = pytest.mark.gpu

WIDE = [(f, b) for f in (5, 64, 129, 260) for b in (0, 1)]
wide = pytest.mark.parametrize("f,bias", WIDE)
GUARD = 4096                                                        # bytes kept past workspace_bytes
GUARD_BYTE = 0xA5
MAX_TOPN = 4096
SMALL_TOPNS = (1, 10, 128, 129, 130, 255, 256, 257, 1000)
LARGE_TOPNS = (4095, 4096)


# ------------------------------------------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=None)
def _factors(f, n_items, cls="exact"):
    """The users of tests/scan_cases.py and a catalogue of n_items rows of the same class.  Computed once, never written."""
    make = ref.exact_factors if cls == "exact" else ref.rounded_factors
    Uf, If = _host(f, cls)[0], make(n_items, f, 10 * f + 3)
    If.setflags(write=False)
    return Uf, If


@functools.lru_cache(maxsize=None)
def _int_scores(f, bias, n_items):
    Uf, If = _factors(f, n_items)
    M = ref.score_matrix_int(Uf, If, np.arange(N_USERS), np.arange(n_items), bias)
    M.setflags(write=False)
    return M


class Wide:
    """wmf_recommend_topn_wide on one user list and one item matrix; any of the three forms (fc.Filtered's arguments)."""

    def __init__(self, Uf, If, f, ld, bias, user_idx):
        self.Ud, self.Id, self.args = _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld)), (f, ld, bias)
        self.user_idx = _dev(user_idx, np.int32)
        self.n_users, self.n_items = len(user_idx), len(If)

    def __call__(self, topn, n_slices, seen=None, bits=None, allow_idx=None, cand=None, expect=None, null=(), **over):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        nu, ni = self.n_users, self.n_items
        cols = max(1, min(topn, MAX_TOPN + 1))
        need = int(lib.wmf_recommend_wide_workspace_bytes(nu, max(1, min(topn, MAX_TOPN)), max(0, min(n_slices, 256))))
        ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        items = torch.full((nu + 2, cols), -7, dtype=torch.int32, device="cuda")        # a sentinel row on either side
        sc = torch.full((nu + 2, cols), fc.SENTINEL, dtype=torch.float32, device="cuda")
        cnt = torch.full((nu + 2,), -7, dtype=torch.int32, device="cuda")
        ip_d = idx_d = bits_d = ai_d = cand_d = None
        if seen is not None:
            indptr, indices = rref.csr_of(seen)
            assert len(indptr) == nu + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        words = n_masks = n_cand = 0
        if bits is not None:
            bits = np.atleast_2d(bits)
            bits_d, (n_masks, words) = _dev(bits.view(np.int32)), bits.shape
        if allow_idx is not None:
            ai_d = _dev(allow_idx, np.int32)
        if cand is not None:
            cand_d, n_cand = _dev(np.append(cand, 0), np.int32), len(cand)
        ptr = {"users": _ptr(self.Ud), "items": _ptr(self.Id), "user_idx": _ptr(self.user_idx), "out_items": _ptr(items[1:]), "workspace": _ptr(ws)}
        for name in null:
            ptr[name] = None
        rc = lib.wmf_recommend_topn_wide(ptr["users"], ptr["items"], f, ld, bias, ptr["user_idx"], nu, ni, _ptr(ip_d), _ptr(idx_d),
                                         _ptr(bits_d), over.get("allow_words", words), over.get("n_masks", n_masks), _ptr(ai_d), _ptr(cand_d),
                                         over.get("n_cand", n_cand), topn, n_slices, ptr["out_items"], _ptr(sc[1:]), _ptr(cnt[1:]), ptr["workspace"],
                                         over.get("ws_bytes", need), _stream())
        items, sc, cnt, tail = items.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy(), ws[need:].cpu().numpy()
        assert (tail == GUARD_BYTE).all(), "the guard region past workspace_bytes was written"
        for a, fill in ((items, -7), (sc, np.float32(fc.SENTINEL)), (cnt, -7)):
            assert (a[0] == fill).all() and (a[-1] == fill).all(), "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (items == -7).all() and (sc == np.float32(fc.SENTINEL)).all() and (cnt == -7).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return items[1:-1], sc[1:-1], cnt[1:-1]


def _check_exact(got, M, users, seen, topn, what, masks=None):
    """Items, scores, counts and padding against the int64 reference; masks: bool [rows, n_items], the complement joins the seen row."""
    items, sc, cnt = got
    want = []
    for b, u in enumerate(users):
        s = np.asarray([] if seen is None else seen[b], dtype=np.int64)
        if masks is not None:
            s = np.concatenate([s, np.flatnonzero(~masks[b])])
        want.append(rref.recommend_ref(M[u], s, topn))
    want_items = rref.padded_rows(want, topn, -1, np.int32)
    assert np.array_equal(items, want_items), (what, np.argwhere(items != want_items)[:5])
    assert np.array_equal(cnt, [len(w) for w in want]), what
    valid = want_items >= 0
    assert (sc[~valid] == -np.inf).all(), what
    assert np.array_equal(sc[valid].astype(np.int64), M[np.repeat(users, valid.sum(axis=1)), want_items[valid]]), what
    assert np.array_equal(sc[valid], np.rint(sc[valid])), what


def _with_complement(seen, masks):
    return [np.sort(np.concatenate([np.asarray(s, dtype=np.int64), np.flatnonzero(~m)])) for s, m in zip(seen, masks)]


# ------------------------------------------------------------------------------------- 1. the table of topn x catalogue sizes
@wide
@pytest.mark.parametrize("n_items", (300, 2000, 2063, 4000, 4096, 4097, 12293))
def test_exact_table(f, bias, n_items):
    """A catalogue shorter than topn, equal to it, just past it, and one that forces several cuts of a buffer (12 293 at 4096:
    a buffer of 8192 keys is cut at least once per slice for the rows that see rising scores)."""
    topns = SMALL_TOPNS if n_items < 4000 else LARGE_TOPNS
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    rng = np.random.default_rng(9000 + 2 * f + bias + n_items)
    seen = _seen_rows(rng, M[users], n_items, n_items % 8)
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    for topn in topns:
        _check_exact(run(topn, 0, seen), M, users, seen, topn, (f, bias, n_items, topn))
    _check_exact(run(topns[-1], 0), M, users, None, topns[-1], (f, bias, n_items, "no seen list"))


@case
def test_every_width_and_leading_dimension_at_129(f, bias, extra):
    ld = _ld(f, extra)
    M, _ = _scores(f, bias, "exact")
    users = _user_list()
    rng = np.random.default_rng(9100 + 2 * f + bias + extra)
    seen = _seen_rows(rng, M[users], N_ITEMS, f % 8)
    run = Wide(*_host(f, "exact"), f, ld, bias, users)
    _check_exact(run(129, 0, seen), M, users, seen, 129, (f, bias, ld))


# --------------------------------------------------------------------------------------------------------- 2. batch sizes
@pytest.mark.parametrize("rows", (1, 15, 16, 17, 33, 65, 129))
def test_batch_sizes(rows):
    """One user twice with two seen rows (positions 2 and 9 from 10 rows on); the eight seen-row patterns in turn."""
    f, bias, n_items = 5, 1, 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list(rows)
    rng = np.random.default_rng(9200 + rows)
    seen = _seen_rows(rng, M[users], n_items, rows)
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    for topn in (129, 1000):
        got = run(topn, 0, seen)
        _check_exact(got, M, users, seen, topn, (rows, topn))
        if rows > 9:
            assert users[2] == users[9] and not np.array_equal(got[0][2], got[0][9])


# ---------------------------------------------------------------------------------------------------- 3. insertion extremes
EXTREMES = ("ascending", "descending", "all equal", "blocks of 17")


@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("shape", EXTREMES)
def test_insertion_extremes(shape, bias):
    """f = 1, or f = 2 with bias: the score is the item's value times the user's factor (plus both biases).  Ascending in the id:
    every item beats the threshold, the most cuts possible; descending: no insertion after the first topn; all equal: the lowest
    ids win; equal in blocks of 17: ties across tile edges.  The users 1, -1, 0 and 2 turn each shape round as well."""
    n = 5000
    j = np.arange(n, dtype=np.int64)
    value = {"ascending": j, "descending": -j, "all equal": 0 * j + 3, "blocks of 17": j // 17}[shape]
    ufac = np.array([1, -1, 0, 2], dtype=np.int64)
    f = 1 + bias
    Uf, If = np.zeros((4, f), dtype=np.float32), np.zeros((n, f), dtype=np.float32)
    Uf[:, -1], If[:, -1] = ufac, value
    if bias:
        Uf[:, 0], If[:, 0] = [0, 5, -2, 1], (j % 3) - 1
    M = ref.score_matrix_int(Uf, If, np.arange(4), j, bias)
    assert np.abs(M).max() < 2 ** 24
    users = np.arange(4)
    seen = [np.arange(0), np.arange(0, n, 2), np.arange(n - 40, n), np.arange(100)]
    run = Wide(Uf, If, f, _ld(f), bias, users)
    for topn in (129, 1000):
        for s in (None, seen):
            _check_exact(run(topn, 0, s), M, users, s, topn, (shape, bias, topn, s is not None))
        _check_exact(run(topn, 1, seen), M, users, seen, topn, (shape, bias, topn, "one slice"))


# --------------------------------------------------------------------------------------------------------------- 4. slices
@pytest.mark.parametrize("f,bias", [(5, 1), (129, 0)])
def test_the_result_does_not_depend_on_the_slices(f, bias):
    n_items = 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    rng = np.random.default_rng(9300 + f)
    seen = _seen_rows(rng, M[users], n_items, 4)
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    for topn in (129, 1000):
        first = run(topn, 0, seen)
        _check_exact(first, M, users, seen, topn, (f, bias, topn))
        assert fc.same_bits(run(topn, 0, seen), first), "two runs, the same bits"
        for n_slices in (1, 2, 3, 7, 64, 256):
            assert fc.same_bits(run(topn, n_slices, seen), first), (f, bias, topn, n_slices)
        for b in (0, 9, 39):                                         # a row alone gives the bits it has in the batch
            alone = Wide(*_factors(f, n_items), f, _ld(f), bias, users[b: b + 1])(topn, 0, seen[b: b + 1])
            assert fc.same_bits(alone, [a[b: b + 1] for a in first]), (f, bias, topn, b)


# ---------------------------------------------------------------------------------------- 5. the launcher's switches, by name
def test_beyond_both_grid_caps():
    """WMF_SCAN_GRID: more (64-row block, slice) pairs than workgroups of the scan; WMF_REC_MERGE_GRID: more rows than workgroups
    of the selection.  Every other test of this file stays below both."""
    f, bias, topn, n_slices, n_items, rows = 5, 1, 129, 256, 4200, 1100
    scan_cap = _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    select_cap = _constant("WMF_REC_MERGE_GRID", "recmodel_amd/csrc/wmf_recommend.hip")
    waves = _constant("WMF_REC_WIDE_WAVES", "recmodel_amd/csrc/wmf_topn_wide.h")
    assert -(-rows // (16 * waves)) * n_slices > scan_cap >= -(-N_USERS // (16 * waves)) * n_slices
    assert rows > select_cap >= 129
    M = _int_scores(f, bias, n_items)
    users = np.arange(rows) % N_USERS
    seen = [np.array([(7 * b) % n_items]) for b in range(rows)]
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    _check_exact(run(topn, n_slices, seen), M, users, seen, topn, "both caps")
    mask = fc.mask_row(6, None, None, None, n_items)
    got = run(topn, n_slices, seen, bits=fc.pack(mask))
    _check_exact(got, M, users, seen, topn, "both caps, mask", np.tile(mask, (rows, 1)))
    assert fc.same_bits(run(topn, n_slices, seen, cand=np.flatnonzero(mask)), got)


def test_both_sides_of_the_automatic_slice_rules():
    """The automatic slice count has three bounds (include/wmf_hip.h): WMF_RECOMMEND_WIDE_AUTO_SLICES, the lists of
    WMF_RECOMMEND_WIDE_AUTO_LISTS (fewer slices from AUTO_LISTS / AUTO_SLICES + 1 rows on) and the slice length max(1024,
    WMF_RECOMMEND_WIDE_SLICE_TOPNS x topn) -- the floor of 1024 up to topn 128, the multiple from 129 on.  A shape on each side of
    each; the answer is the reference's on all of them, and that of one slice."""
    h = "include/wmf_hip.h"
    auto, lists, per = (_constant(n, h) for n in ("WMF_RECOMMEND_WIDE_AUTO_SLICES", "WMF_RECOMMEND_WIDE_AUTO_LISTS", "WMF_RECOMMEND_WIDE_SLICE_TOPNS"))
    assert per * 128 <= 1024 < per * 129
    f, bias = 5, 1
    edge = lists // auto                                            # 512 rows: still AUTO_SLICES slices
    n_long = 1024 * auto + 16                                       # long enough that the slice length binds nowhere at topn <= 128
    # (rows, items, topn): the bound that decides
    shapes = [(N_USERS, 300, 128), (N_USERS, 300, 129),             # one slice: the catalogue is shorter than a slice
              (N_USERS, 2063, 128), (N_USERS, 2063, 129),           # the slice length: 1024 items, then 8 x 129
              (N_USERS, n_long, 10),                                # AUTO_SLICES
              (edge, n_long, 10), (edge + 1, n_long, 10)]           # the lists: 64 slices at 512 rows, 63 at 513
    for rows, n_items, topn in shapes:
        M = _int_scores(f, bias, n_items)
        users = np.arange(rows) % N_USERS
        run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
        got = run(topn, 0)
        head = [a[:N_USERS] for a in got]
        _check_exact(head, M, users[:N_USERS], None, topn, (rows, n_items, topn))
        for b in range(N_USERS, rows):                              # without seen rows a position's answer is its user's
            assert all(np.array_equal(a[b], a[b % N_USERS]) for a in got), (rows, n_items, topn, b)


@pytest.mark.parametrize("f", (64, 65, 144, 145))
def test_both_sides_of_the_width_classes(f):
    """ld 64 | 68: four or five trips of the feature loop (the classes <4, 4> and <9, 2>); ld 144 | 148: nine or ten (<9, 2> and
    <17, 1>).  The kernel's name says which class ran."""
    n_items, topn = 2063, 1000
    M = _int_scores(f, 1, n_items)
    users = _user_list()
    run = Wide(*_factors(f, n_items), f, _ld(f), 1, users)
    names = _launched(lambda: _check_exact(run(topn, 0), M, users, None, topn, f))
    cls = {64: "4, 4", 65: "9, 2", 144: "9, 2", 145: "17, 1"}[f]
    assert names == {f"recommend_scan_wide_kernel<{cls}, 4>", "recommend_select_wide_kernel"}


# -------------------------------------------------------------------------------------------------------------- 6. filters
@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
@pytest.mark.parametrize("topn", (129, 1000))
def test_mask_form(f, bias, topn):
    """The twelve patterns of tests/filter_cases.py: equal to the unfiltered wide call with the complement in the seen rows, bit
    for bit, and to the reference."""
    n_items = 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    for pattern in range(len(fc.PATTERNS)):
        rng = np.random.default_rng(9400 + 100 * pattern + f)
        seen = _seen_rows(rng, M[users], n_items, pattern)
        masks = fc.mask_rows(pattern, rng, M[users], seen, n_items)
        bits, allow_idx = fc.bits_of(pattern, masks)
        got = run(topn, 0, seen, bits=bits, allow_idx=allow_idx)
        what = (f, bias, topn, fc.PATTERNS[pattern])
        assert fc.same_bits(got, run(topn, 0, _with_complement(seen, masks))), what
        _check_exact(got, M, users, seen, topn, what, masks)


@pytest.mark.parametrize("topn", (129, 1000))
def test_per_row_masks(topn):
    """Four masks, allow_idx cycling -1, 0, 1, 2, 3: user 2 stands at positions 2 and 9 under masks 1 and 3."""
    f, bias, n_items = 5, 1, 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    rng = np.random.default_rng(9500)
    seen = _seen_rows(rng, M[users], n_items, 3)
    G = np.stack([fc.mask_row(p, rng, M[0], [], n_items) for p in (9, 6, 5, 7)])
    allow_idx = np.arange(N_USERS) % 5 - 1
    assert allow_idx[2] == 1 and allow_idx[9] == 3 and users[2] == users[9]
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    got = run(topn, 0, seen, bits=fc.pack(G), allow_idx=allow_idx)
    masks = np.where(allow_idx[:, None] < 0, True, G[allow_idx])
    assert fc.same_bits(got, run(topn, 0, _with_complement(seen, masks)))
    _check_exact(got, M, users, seen, topn, "per-row masks", masks)
    assert not np.array_equal(got[0][2], got[0][9])


@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
def test_list_form(f, bias):
    """Lists of 1, 15, 16, 17, 33, 300 and 3000 ids: the unfiltered wide call with the complement seen, and the mask form of the
    same list, bit for bit."""
    n_items = 4200
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    rng = np.random.default_rng(9600 + f)
    seen = _seen_rows(rng, M[users], n_items, 5)
    run = Wide(*_factors(f, n_items), f, _ld(f), bias, users)
    for n in (1, 15, 16, 17, 33, 300, 3000):
        cand = np.sort(rng.choice(n_items, n, replace=False))
        if n > 1:
            cand[0], cand[-1] = 0, n_items - 1
        mask = np.isin(np.arange(n_items), cand)
        masks = np.tile(mask, (N_USERS, 1))
        for topn in (129, 1000):
            got = run(topn, 0, seen, cand=cand)
            assert fc.same_bits(got, run(topn, 0, seen, bits=fc.pack(mask))), (f, bias, n, topn, "mask form")
            assert fc.same_bits(got, run(topn, 0, _with_complement(seen, masks))), (f, bias, n, topn, "complement seen")
            _check_exact(got, M, users, seen, topn, (f, bias, n, topn), masks)


# --------------------------------------------------------------------------------------------- 7. against the old kernels
@wide
@pytest.mark.parametrize("cls", ("exact", "rounded"))
def test_up_to_128_the_wide_kernels_give_the_bits_of_the_old_ones(f, bias, cls):
    ld = _ld(f)
    users = _user_list()
    S, _ = _scores(f, bias, cls)
    rng = np.random.default_rng(9700 + 2 * f + bias)
    seen = _seen_rows(rng, S[users], N_ITEMS, 2)
    mask = fc.mask_row(9, rng, None, None, N_ITEMS)
    cand = np.flatnonzero(mask)
    new, old, plain = Wide(*_host(f, cls), f, ld, bias, users), fc.Filtered(*_host(f, cls), f, ld, bias, users), _Recommend(*_host(f, cls), f, ld, bias, users)
    for topn in (1, 10, 128):
        assert fc.same_bits(new(topn, 0, seen), plain(N_USERS, N_ITEMS, topn, 0, seen)), (f, bias, cls, topn)
        assert fc.same_bits(new(topn, 0, seen, bits=fc.pack(mask)), old(topn, 0, seen, bits=fc.pack(mask))), (f, bias, cls, topn, "mask")
        assert fc.same_bits(new(topn, 0, seen, cand=cand), old(topn, 0, seen, cand=cand)), (f, bias, cls, topn, "list")


def _device_scores(run, n_users_model, n_items):
    """float32 [users of the model, n_items]: the scores wmf_rank_topn_batch returns for the whole catalogue as the candidate list,
    put back in item order -- the 16 x 16 tile's arithmetic, bit for bit the scan's (include/wmf_hip.h; wmf_predict_pairs sums in
    another order and differs in the last bits)."""
    _lib, lib, _ptr, _stream = _api()
    f, ld, bias = run.args
    uu, cand = _dev(np.arange(n_users_model), np.int32), _dev(np.arange(n_items), np.int32)
    ws = torch.empty(int(lib.wmf_rank_batch_workspace_bytes(n_users_model, n_items)), dtype=torch.uint8, device="cuda")
    pos = torch.empty(n_users_model * n_items, dtype=torch.int32, device="cuda")
    sc = torch.empty(n_users_model * n_items, dtype=torch.float32, device="cuda")
    _lib.check(lib.wmf_rank_topn_batch(_ptr(run.Ud), _ptr(run.Id), f, ld, bias, _ptr(uu), n_users_model, _ptr(cand), n_items, n_items, _ptr(pos),
                                       _ptr(sc), _ptr(ws), ws.numel(), _stream()))
    pos, sc = pos.cpu().numpy().reshape(n_users_model, n_items), sc.cpu().numpy().reshape(n_users_model, n_items)
    D = np.empty_like(sc)
    np.put_along_axis(D, pos.astype(np.int64), sc, axis=1)
    return D


@wide
def test_topn_1000_on_gaussian_factors(f, bias):
    """The first 128 columns are wmf_recommend_topn's at 128; the whole row is the host top-n of the device's own scores."""
    n_items, topn = 2063, 1000
    Uf, If = _factors(f, n_items, "rounded")
    users = _user_list()
    run, plain = Wide(Uf, If, f, _ld(f), bias, users), _Recommend(Uf, If, f, _ld(f), bias, users)
    D = _device_scores(run, N_USERS, n_items)
    rng = np.random.default_rng(9800 + f)
    seen = _seen_rows(rng, D[users].astype(np.float64), n_items, 6)
    items, sc, cnt = run(topn, 0, seen)
    first = plain(N_USERS, n_items, 128, 0, seen)
    assert fc.same_bits((items[:, :128], sc[:, :128]), first[:2]) and np.array_equal(np.minimum(cnt, 128), first[2])
    want = [rref.recommend_ref(D[u], seen[b], topn) for b, u in enumerate(users)]
    want_items = rref.padded_rows(want, topn, -1, np.int32)
    assert np.array_equal(items, want_items) and np.array_equal(cnt, [len(w) for w in want])
    valid = want_items >= 0
    assert (sc[~valid] == -np.inf).all()
    assert np.array_equal(sc[valid].view(np.int32), D[np.repeat(users, valid.sum(axis=1)), want_items[valid]].view(np.int32))


# ----------------------------------------------------------------------------------------------------- 8. which kernel ran
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


def test_the_wide_call_runs_only_wide_kernels_and_the_old_calls_only_the_old_ones():
    f, bias = 5, 1
    ld = _ld(f)
    users = _user_list()
    new, old, plain = (c(*_host(f, "exact"), f, ld, bias, users) for c in (Wide, fc.Filtered, _Recommend))
    mask = fc.mask_row(6, None, None, None, N_ITEMS)
    cand = np.flatnonzero(mask)
    select = "recommend_select_wide_kernel"
    for topn in (10, 129, 4096):
        assert _launched(lambda: new(topn, 0)) == {"recommend_scan_wide_kernel<4, 4, 4>", select}
        assert _launched(lambda: new(topn, 0, bits=fc.pack(mask))) == {"recommend_scan_wide_mask_kernel<4, 4, 4>", select}
        assert _launched(lambda: new(topn, 0, cand=cand)) == {"recommend_scan_wide_list_kernel<4, 4, 4>", select}
    assert _launched(lambda: plain(N_USERS, N_ITEMS, 10, 0)) == {"recommend_scan_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: old(10, 0)) == {"recommend_scan_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: old(10, 0, bits=fc.pack(mask))) == {"recommend_scan_mask_kernel<4, 4, 4>", "recommend_merge_kernel"}
    assert _launched(lambda: old(128, 0, cand=cand)) == {"recommend_scan_list_kernel<4, 4, 2>", "recommend_merge_kernel"}


# -------------------------------------------------------------------------------------------------------- 9. WMF_EINVAL
def test_refusals_come_before_any_launch():
    _lib = _api()[0]
    f, bias = 5, 1
    run, old = (c(*_host(f, "exact"), f, _ld(f), bias, _user_list()) for c in (Wide, fc.Filtered))
    bits, cand = fc.pack(fc.mask_row(6, None, None, None, N_ITEMS)), np.arange(0, N_ITEMS, 3)
    assert bits.shape == (1, 10)
    E = _lib.WMF_EINVAL

    def refused():
        run(0, 0, expect=E)
        run(MAX_TOPN + 1, 0, expect=E)
        run(129, 0, bits=bits, cand=cand, expect=E)                  # both forms in one call
        run(129, 0, bits=bits, n_masks=0, expect=E)
        run(129, 0, bits=bits, allow_words=9, expect=E)              # 300 items need 10 words
        run(129, 0, allow_idx=np.zeros(N_USERS), expect=E)           # allow_idx without bits
        run(129, 0, cand=cand, n_cand=0, expect=E)
        run(129, 0, cand=cand, n_cand=N_ITEMS + 1, expect=E)
        run(129, -1, expect=E)
        run(129, 257, expect=E)
        for form in ({}, {"bits": bits}, {"cand": cand}):
            need = int(_api()[1].wmf_recommend_wide_workspace_bytes(N_USERS, 129, 0))
            run(129, 0, ws_bytes=need - 1, expect=E, **form)         # one byte short
        for name in ("users", "items", "user_idx", "out_items", "workspace"):
            run(129, 0, null=(name,), expect=E)
        old(129, 0, expect=E)                                        # the old entry points keep their limit
    assert _launched(refused) == set()
