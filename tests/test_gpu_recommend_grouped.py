"""wmf_recommend_topn_grouped through the C ABI, per element: one list per (row, group) from one scan of the catalogue.

The reference is tests/grouped_ref.py on the host (list (b, g) = tests/recommend_ref.py with the other groups' items, the items a
mask bars and the row's seen items left out) for the EXACT class, and for both classes wmf_recommend_topn_filtered on the same
device buffers with every row repeated once per group under the groups' masks.  Every comparison is for equality.  Every call keeps
a guard region past its workspace and a sentinel row on either side of its outputs."""
import numpy as np
import pytest
import torch

import filter_cases as fc
import grouped_ref as gref
import recommend_ref as rref
import serving_ref as ref
from scan_cases import LD_EXTRA, N_ITEMS, N_USERS, _api, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list
from test_gpu_recommend_wide import Wide, _factors, _int_scores, _launched

pytestmark = pytest.mark.gpu

GUARD = 4096                                                        # bytes kept past workspace_bytes
GUARD_BYTE = 0xA5
INT32_MAX = 2 ** 31 - 1
GROUP_COUNTS = (1, 2, 3, 31, 32, 33, 64)
TOPNS = (1, 10, 127, 128)


# ------------------------------------------------------------------------------------------------------------- plumbing
class Grouped:
    """wmf_recommend_topn_grouped on one user list and one item matrix."""

    def __init__(self, Uf, If, f, ld, bias, user_idx):
        self.host = (Uf, If)
        self.Ud, self.Id, self.args = _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld)), (f, ld, bias)
        self.users = np.asarray(user_idx)
        self.user_idx = _dev(user_idx, np.int32)
        self.n_users, self.n_items = len(user_idx), len(If)

    def __call__(self, group_of, G, topn, n_slices=0, seen=None, bits=None, allow_idx=None, expect=None, null=(), **over):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        nu, ni = self.n_users, self.n_items
        g_ok, t_ok = max(1, min(G, 64)), max(1, min(topn, 128))      # (the shapes of a call that is to be refused)
        need = int(lib.wmf_recommend_grouped_workspace_bytes(nu, g_ok, t_ok, max(0, min(n_slices, 256))))
        ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        items = torch.full((nu + 2, g_ok * t_ok), -7, dtype=torch.int32, device="cuda")     # a sentinel row on either side
        sc = torch.full((nu + 2, g_ok * t_ok), fc.SENTINEL, dtype=torch.float32, device="cuda")
        cnt = torch.full((nu + 2, g_ok), -7, dtype=torch.int32, device="cuda")
        assert len(group_of) == ni
        g_d = _dev(group_of, np.int32)
        ip_d = idx_d = bits_d = ai_d = None
        if seen is not None:
            indptr, indices = rref.csr_of(seen)
            assert len(indptr) == nu + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        words = n_masks = 0
        if bits is not None:
            bits = np.atleast_2d(bits)
            bits_d, (n_masks, words) = _dev(bits.view(np.int32)), bits.shape
        if allow_idx is not None:
            ai_d = _dev(allow_idx, np.int32)
        ptr = {"users": _ptr(self.Ud), "items": _ptr(self.Id), "user_idx": _ptr(self.user_idx), "out_items": _ptr(items[1:]), "workspace": _ptr(ws),
               "group_of": _ptr(g_d)}
        for name in null:
            ptr[name] = None
        rc = lib.wmf_recommend_topn_grouped(ptr["users"], ptr["items"], f, ld, bias, ptr["user_idx"], nu, ni, _ptr(ip_d), _ptr(idx_d), _ptr(bits_d),
                                            over.get("allow_words", words), over.get("n_masks", n_masks), _ptr(ai_d), ptr["group_of"], G, topn,
                                            n_slices, ptr["out_items"], _ptr(sc[1:]), _ptr(cnt[1:]), ptr["workspace"], over.get("ws_bytes", need),
                                            _stream())
        items, sc, cnt, tail = items.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy(), ws[need:].cpu().numpy()
        assert (tail == GUARD_BYTE).all(), "the guard region past workspace_bytes was written"
        for a, fill in ((items, -7), (sc, np.float32(fc.SENTINEL)), (cnt, -7)):
            assert (a[0] == fill).all() and (a[-1] == fill).all(), "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (items == -7).all() and (sc == np.float32(fc.SENTINEL)).all() and (cnt == -7).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return items[1:-1].reshape(nu, G, topn), sc[1:-1].reshape(nu, G, topn), cnt[1:-1]


def _check_exact(got, M, users, seen, group_of, G, topn, what, masks=None):
    """Items, scores, counts and padding of every list against the int64 reference; masks: bool [rows, n_items] or None."""
    items, sc, cnt = got
    for b, u in enumerate(users):
        lists = gref.grouped_ref(M[u], [] if seen is None else seen[b], group_of, G, topn, None if masks is None else masks[b])
        want = rref.padded_rows(lists, topn, -1, np.int32)
        assert np.array_equal(items[b], want), (what, b, np.argwhere(items[b] != want)[:5])
        assert np.array_equal(cnt[b], [len(w) for w in lists]), (what, b)
        valid = want >= 0
        assert (sc[b][~valid] == -np.inf).all(), (what, b)
        assert np.array_equal(sc[b][valid].astype(np.int64), M[u, want[valid]]) and np.array_equal(sc[b][valid], np.rint(sc[b][valid])), (what, b)


def _check_filtered(run, got, group_of, G, topn, seen, what, masks=None):
    """Bit for bit wmf_recommend_topn_filtered on the same device buffers, every row repeated once per group under the group's mask
    (and the row's own)."""
    nu = run.n_users
    of_group = np.stack([np.asarray(group_of) == g for g in range(G)])
    if masks is None:
        bits, allow_idx = fc.pack(of_group), np.tile(np.arange(G), nu)
    else:
        bits, allow_idx = fc.pack((masks[:, None, :] & of_group[None]).reshape(nu * G, -1)), np.arange(nu * G)
    old = fc.Filtered(*run.host, *run.args, np.repeat(run.users, G))
    old.Ud, old.Id = run.Ud, run.Id
    rows = None if seen is None else [seen[b] for b in range(nu) for _ in range(G)]
    want = old(topn, 0, rows, bits=bits, allow_idx=allow_idx)
    assert fc.same_bits((got[0].reshape(nu * G, topn), got[1].reshape(nu * G, topn), got[2].reshape(-1)), want), what


def _mod(G, n=N_ITEMS):
    return np.arange(n) % G


# ------------------------------------------------------------------------------------ 1. widths, biases, leading dimensions
@pytest.mark.parametrize("f,bias,extra", [(f, b, e) for f in (5, 64, 129, 260) for b in (0, 1) for e in (0, LD_EXTRA[f])])
def test_every_width_class_bias_and_leading_dimension(f, bias, extra):
    ld, G, topn = _ld(f, extra), 3, 10
    users = _user_list()
    group_of = np.where(np.arange(N_ITEMS) % 11 == 10, -1, _mod(G))
    for cls in ("exact", "rounded"):
        S, _ = _scores(f, bias, cls)
        rng = np.random.default_rng(11000 + 2 * f + bias + extra)
        seen = _seen_rows(rng, S[users], N_ITEMS, f % 8)
        run = Grouped(*_host(f, cls), f, ld, bias, users)
        got = run(group_of, G, topn, 0, seen)
        if cls == "exact":
            _check_exact(got, S, users, seen, group_of, G, topn, (f, bias, ld))
        _check_filtered(run, got, group_of, G, topn, seen, (f, bias, ld, cls))


# -------------------------------------------------------------------------------------------------- 2. group counts and topn
@pytest.mark.parametrize("G", GROUP_COUNTS)
def test_group_counts_and_topn(G):
    f, bias = 5, 1
    users = _user_list()
    M, _ = _scores(f, bias, "exact")
    rng = np.random.default_rng(11100 + G)
    seen = _seen_rows(rng, M[users], N_ITEMS, G)
    run, rounded = Grouped(*_host(f, "exact"), f, _ld(f), bias, users), Grouped(*_host(f, "rounded"), f, _ld(f), bias, users)
    group_of = rng.integers(0, G, N_ITEMS)
    for topn in TOPNS:
        got = run(group_of, G, topn, 0, seen)
        _check_exact(got, M, users, seen, group_of, G, topn, (G, topn))
        _check_filtered(run, got, group_of, G, topn, seen, (G, topn))
        _check_filtered(rounded, rounded(group_of, G, topn, 0, seen), group_of, G, topn, seen, (G, topn, "rounded"))


# ---------------------------------------------------------------------------------------------------------- 3. group patterns
def _patterns(seen):
    """name -> (group_of, G, n_slices).  300 items in three slices: 19 tiles, seven per slice, a slice edge at item 112."""
    j = np.arange(N_ITEMS)
    out = {"j % G": (j % 5, 5, 0),
           "blocks with edges at 15, 16, 17 and the slice edge": (np.searchsorted([15, 16, 17, 112, 200], j, side="right"), 6, 3),
           "one group owns whole tiles": (np.where((j // 16) % 2 == 0, 0, 1 + j % 3), 4, 0),
           "everything in one group": (np.full(N_ITEMS, 2), 4, 0),
           "every item on no shelf": (np.full(N_ITEMS, -1), 3, 0),
           "an empty group": (np.where(j % 3 == 1, 3, j % 3), 4, 0),
           "groups smaller than topn": (np.where(j < 7, 0, np.where(j < 16, 1, np.where(j > 290, 2, 3))), 4, 0),
           "-1, -7, n_groups and INT32_MAX are no shelf": (np.choose(j % 6, [0, -1, 1, -7, 2, INT32_MAX]) + np.where(j % 12 == 0, 3, 0), 3, 0)}
    only_seen = np.ones(N_ITEMS, dtype=np.int64)
    only_seen[seen[3]] = 0                                          # group 0 holds exactly the items row 3 has seen
    out["one group holds only a row's seen items"] = (only_seen, 2, 0)
    return out


PATTERN_NAMES = tuple(_patterns([np.zeros(0, dtype=int)] * 4))


@pytest.mark.parametrize("name", PATTERN_NAMES)
def test_group_patterns(name):
    f, bias = 5, 1
    users = _user_list()
    M, _ = _scores(f, bias, "exact")
    rng = np.random.default_rng(11200)
    seen = _seen_rows(rng, M[users], N_ITEMS, 0)                    # row 3: one whole 16-item tile
    assert len(seen[3]) == 16
    group_of, G, n_slices = _patterns(seen)[name]
    run = Grouped(*_host(f, "exact"), f, _ld(f), bias, users)
    for topn in (1, 10, 128):
        got = run(group_of, G, topn, n_slices, seen)
        _check_exact(got, M, users, seen, group_of, G, topn, (name, topn))
        _check_filtered(run, got, np.where((group_of < 0) | (group_of >= G), -1, group_of), G, topn, seen, (name, topn))
        if name == "one group holds only a row's seen items":
            assert got[2][3, 0] == 0 and (got[0][3, 0] == -1).all() and len(seen[0]) == 0 and got[2][0, 0] == min(topn, 16)
        if name == "every item on no shelf":
            assert (got[2] == 0).all() and (got[0] == -1).all() and (got[1] == -np.inf).all()
        if name == "groups smaller than topn":
            assert got[2][0].tolist() == [min(topn, 7), min(topn, 9), min(topn, 9), min(topn, 128)]


# -------------------------------------------------------------------------------------------------------- 4. insertion extremes
@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("shape", ("ascending", "descending", "all equal", "blocks of 17"))
def test_insertion_extremes(shape, bias):
    """The score is the item's value times the user's factor (plus both biases).  Ascending in the id: every item beats its
    group's threshold, the most cuts possible -- and with a group that owns whole tiles, 16 appends to one buffer in one tile, the
    cap - 16 bound at topn 1 and 10 (cap 32: a cut every other tile); descending: no insertion after a group's first topn; all
    equal: the lowest ids of every group win; equal in blocks of 17: ties across tile edges, within and across groups."""
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
    users = np.arange(4)
    seen = [np.arange(0), np.arange(0, n, 2), np.arange(n - 40, n), np.arange(100)]
    run = Grouped(Uf, If, f, _ld(f), bias, users)
    for group_of, G in ((np.zeros(n, dtype=np.int64), 1), (j % 5, 5), (np.where((j // 16) % 2 == 0, 0, 1 + j % 2), 3)):
        for topn in (1, 10, 128):
            for n_slices in (0, 1):
                _check_exact(run(group_of, G, topn, n_slices, seen), M, users, seen, group_of, G, topn, (shape, bias, G, topn, n_slices))
        _check_filtered(run, run(group_of, G, 10, 0, seen), group_of, G, 10, seen, (shape, bias, G))


# ------------------------------------------------------------------------------------------------------------ 5. the mask form
def test_mask_form_one_mask_and_one_per_row():
    """Four masks, allow_idx cycling -1, 0, 1, 2, 3: user 2 stands at positions 2 and 9 under masks 1 and 3."""
    f, bias, G, topn = 5, 1, 4, 10
    users = _user_list()
    M, _ = _scores(f, bias, "exact")
    rng = np.random.default_rng(11300)
    seen = _seen_rows(rng, M[users], N_ITEMS, 3)
    group_of = np.where(np.arange(N_ITEMS) % 13 == 0, -1, _mod(G))
    run, rounded = Grouped(*_host(f, "exact"), f, _ld(f), bias, users), Grouped(*_host(f, "rounded"), f, _ld(f), bias, users)
    for pattern in (6, 9, 10, 11, 1):                               # every other, random 30 %, random 1 %, dead bits set, nothing
        mask = fc.mask_row(pattern, rng, M[0], [], N_ITEMS)
        masks = np.tile(mask, (N_USERS, 1))
        got = run(group_of, G, topn, 0, seen, bits=fc.pack(mask, fc.PATTERNS[pattern] == "dead bits set"))
        _check_exact(got, M, users, seen, group_of, G, topn, fc.PATTERNS[pattern], masks)
        _check_filtered(run, got, group_of, G, topn, seen, fc.PATTERNS[pattern], masks)
    four = np.stack([fc.mask_row(p, rng, M[0], [], N_ITEMS) for p in (9, 6, 5, 7)])
    allow_idx = np.arange(N_USERS) % 5 - 1
    assert allow_idx[2] == 1 and allow_idx[9] == 3 and users[2] == users[9]
    masks = np.where(allow_idx[:, None] < 0, True, four[allow_idx])
    for r in (run, rounded):
        got = r(group_of, G, topn, 0, seen, bits=fc.pack(four), allow_idx=allow_idx)
        _check_filtered(r, got, group_of, G, topn, seen, "per-row masks", masks)
    _check_exact(got := run(group_of, G, topn, 0, seen, bits=fc.pack(four), allow_idx=allow_idx), M, users, seen, group_of, G, topn, "per-row masks", masks)
    assert not np.array_equal(got[0][2], got[0][9])


# ---------------------------------------------------------------------------------------------------------------- 6. batches
@pytest.mark.parametrize("rows", (1, 15, 16, 17, 63, 64, 65))
def test_batch_sizes(rows):
    """One user twice with two seen rows (positions 2 and 9 from 10 rows on); the eight seen-row patterns in turn."""
    f, bias, G, topn = 5, 1, 3, 10
    M, _ = _scores(f, bias, "exact")
    users = _user_list(rows)
    rng = np.random.default_rng(11400 + rows)
    seen = _seen_rows(rng, M[users], N_ITEMS, rows)
    run = Grouped(*_host(f, "exact"), f, _ld(f), bias, users)
    got = run(_mod(G), G, topn, 0, seen)
    _check_exact(got, M, users, seen, _mod(G), G, topn, rows)
    _check_filtered(run, got, _mod(G), G, topn, seen, rows)
    if rows > 9:
        assert users[2] == users[9] and not np.array_equal(got[0][2], got[0][9])


# ----------------------------------------------------------------------------------------------------------------- 7. slices
@pytest.mark.parametrize("f,bias,cls", [(5, 1, "exact"), (129, 0, "rounded")])
def test_the_result_does_not_depend_on_the_slices(f, bias, cls):
    n_items, G = 2063, 5
    users = _user_list()
    rng = np.random.default_rng(11500 + f)
    seen = [np.sort(rng.choice(n_items, 30, replace=False)) for _ in users]
    group_of = rng.integers(-1, G, n_items)
    run = Grouped(*_factors(f, n_items, cls), f, _ld(f), bias, users)
    for topn in (10, 128):
        first = run(group_of, G, topn, 0, seen)
        if cls == "exact":
            _check_exact(first, _int_scores(f, bias, n_items), users, seen, group_of, G, topn, (f, topn))
        assert fc.same_bits(run(group_of, G, topn, 0, seen), first), "two runs, the same bits"
        for n_slices in (1, 2, 3, 7, 64, 256):
            assert fc.same_bits(run(group_of, G, topn, n_slices, seen), first), (f, bias, topn, n_slices)


# ------------------------------------------------------------------------------------------- 8. one group is the wide call
@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
@pytest.mark.parametrize("cls", ("exact", "rounded"))
def test_one_group_of_everything_is_the_unfiltered_wide_call(f, bias, cls):
    users = _user_list()
    S, _ = _scores(f, bias, cls)
    rng = np.random.default_rng(11600 + f)
    seen = _seen_rows(rng, S[users], N_ITEMS, 5)
    run, wide = Grouped(*_host(f, cls), f, _ld(f), bias, users), Wide(*_host(f, cls), f, _ld(f), bias, users)
    for topn in TOPNS:
        items, sc, cnt = run(np.zeros(N_ITEMS, dtype=np.int64), 1, topn, 0, seen)
        assert fc.same_bits((items[:, 0], sc[:, 0], cnt[:, 0]), wide(topn, 0, seen)), (f, bias, cls, topn)


# ------------------------------------------------------------------------------------------------------- 9. the grid caps
def test_beyond_the_selection_grid():
    """40 rows x 32 groups: more virtual rows than workgroups of the selection (WMF_REC_MERGE_GRID)."""
    f, bias, G, topn = 5, 1, 32, 10
    assert N_USERS * G > _constant("WMF_REC_MERGE_GRID", "recmodel_amd/csrc/wmf_recommend.hip")
    M, _ = _scores(f, bias, "exact")
    users = _user_list()
    run = Grouped(*_host(f, "exact"), f, _ld(f), bias, users)
    _check_exact(run(_mod(G), G, topn, 0), M, users, None, _mod(G), G, topn, "selection grid")


def test_beyond_the_scan_grid():
    """1040 rows x 256 slices: more (64-row block, slice) pairs than workgroups of the scan (WMF_SCAN_GRID)."""
    f, bias, G, topn, n_slices, n_items, rows = 5, 1, 2, 1, 256, 4200, 1040
    waves = _constant("WMF_REC_WIDE_WAVES", "recmodel_amd/csrc/wmf_topn_wide.h")
    assert -(-rows // (16 * waves)) * n_slices > _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    M = _int_scores(f, bias, n_items)
    users = np.arange(rows) % N_USERS
    seen = [np.array([(7 * b) % n_items]) for b in range(rows)]
    run = Grouped(*_factors(f, n_items), f, _ld(f), bias, users)
    _check_exact(run(_mod(G, n_items), G, topn, n_slices, seen), M, users, seen, _mod(G, n_items), G, topn, "scan grid")


# ----------------------------------------------------------------------------------------------------- 10. which kernel ran
@pytest.mark.parametrize("f", (64, 65, 144, 145))
def test_which_kernels_ran(f):
    users = _user_list()
    run = Grouped(*_factors(f, N_ITEMS), f, _ld(f), 1, users)
    cls = {64: "4, 4", 65: "9, 2", 144: "9, 2", 145: "17, 1"}[f]
    group_of, mask = _mod(7), fc.mask_row(6, None, None, None, N_ITEMS)
    assert _launched(lambda: run(group_of, 7, 10)) == {f"recommend_scan_grouped_kernel<{cls}, 4>", "recommend_select_wide_kernel"}
    assert _launched(lambda: run(group_of, 7, 10, bits=fc.pack(mask))) == {f"recommend_scan_grouped_mask_kernel<{cls}, 4>", "recommend_select_wide_kernel"}


# -------------------------------------------------------------------------------------------------------- 11. WMF_EINVAL
def test_refusals_come_before_any_launch_and_leave_the_outputs_alone():
    _lib, lib = _api()[:2]
    f, bias, G = 5, 1, 4
    run = Grouped(*_host(f, "exact"), f, _ld(f), bias, _user_list())
    group_of, bits = _mod(G), fc.pack(fc.mask_row(6, None, None, None, N_ITEMS))
    assert bits.shape == (1, 10)
    E = _lib.WMF_EINVAL

    def refused():
        for G_bad in (0, -1, 65):
            run(group_of, G_bad, 10, expect=E)
        for topn in (0, 129):
            run(group_of, G, topn, expect=E)
        run(group_of, G, 10, -1, expect=E)
        run(group_of, G, 10, 257, expect=E)
        run(group_of, G, 10, bits=bits, n_masks=0, expect=E)
        run(group_of, G, 10, bits=bits, allow_words=9, expect=E)      # 300 items need 10 words
        run(group_of, G, 10, allow_idx=np.zeros(N_USERS), expect=E)   # allow_idx without bits
        for form in ({}, {"bits": bits}):
            run(group_of, G, 10, ws_bytes=int(lib.wmf_recommend_grouped_workspace_bytes(N_USERS, G, 10, 0)) - 1, expect=E, **form)
        for name in ("users", "items", "user_idx", "out_items", "workspace", "group_of"):
            run(group_of, G, 10, null=(name,), expect=E)
    assert _launched(refused) == set()
