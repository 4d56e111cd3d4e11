"""wmf_sample_topn, wmf_sample_noise and wmf_log_partition through the C ABI, per element, in the vocabulary of
tests/test_gpu_recommend_wide.py.

The noise is held to tests/sample_ref.py bit for bit (the 23 bits of the hash) and to four units in the last place (g).  The EXACT
class makes the sampled list exact as well: integer scores, a power-of-two temperature and the device's own float32 noise (read back
through wmf_sample_noise) give z = fmaf(T, g, score) as the correctly rounded exact sum, so items, key bits, score bits, counts and
padding are compared for equality.  Every call keeps a guard region past its workspace and a sentinel row on either side of its
outputs."""
import math

import numpy as np
import pytest
import torch

import filter_cases as fc
import recommend_ref as rref
import sample_ref as sref
import serving_ref as ref
from conftest import record_error
from scan_cases import LD_EXTRA, N_ITEMS, N_USERS, _api, _constant, _dev, _host, _ld, _scores, _seen_rows, _user_list
from test_gpu_recommend_wide import GUARD, GUARD_BYTE, MAX_TOPN, Wide, _factors, _int_scores, _launched, _with_complement, wide
from test_sample_cpu import CHI_SCORES, CHI_SEED, CHI_STREAMS, CHI_TEMPERATURES, chi_square_gate

pytestmark = pytest.mark.gpu

TEMPS = (0.25, 1.0, 4.0)
NS = (1, 10, 128, 129, 1000)
U64 = 2 ** 64 - 1


# ------------------------------------------------------------------------------------------------------------- plumbing
def _noise(seed, streams, items):
    """(g float32, k uint32) of the pairs (streams[i], items[i]) from wmf_sample_noise; streams None: the pair's index."""
    _lib, lib, _ptr, _stream = _api()
    n = len(items)
    s_d = None if streams is None else _dev(np.asarray(streams, dtype=np.uint64).view(np.int64))
    i_d = _dev(np.asarray(items, dtype=np.int64).astype(np.uint32).view(np.int32))
    g = torch.full((n + 2,), fc.SENTINEL, dtype=torch.float32, device="cuda")
    k = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_sample_noise(seed, _ptr(s_d), _ptr(i_d), n, _ptr(g[1:]), _ptr(k[1:]), _stream()))
    g, k = g.cpu().numpy(), k.cpu().numpy()
    assert g[0] == g[-1] == np.float32(fc.SENTINEL) and k[0] == k[-1] == -7
    return g[1:-1], k[1:-1].view(np.uint32)


def _noise_rows(seed, streams, n_items):
    """float32 [len(streams), n_items]: the device's g of every (stream, item)."""
    streams = np.asarray(streams, dtype=np.uint64)
    g, _ = _noise(seed, np.repeat(streams, n_items), np.tile(np.arange(n_items), len(streams)))
    return g.reshape(len(streams), n_items)


class Sample(Wide):
    """wmf_sample_topn (and wmf_log_partition: logz) on one user list and one item matrix; the filter arguments of Wide."""

    def _filter(self, seen, bits, allow_idx, cand):
        ip_d = idx_d = bits_d = ai_d = cand_d = None
        if seen is not None:
            indptr, indices = rref.csr_of(seen)
            assert len(indptr) == self.n_users + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        words = n_masks = n_cand = 0
        if bits is not None:
            bits = np.atleast_2d(bits)
            bits_d, (n_masks, words) = _dev(bits.view(np.int32)), bits.shape
        if allow_idx is not None:
            ai_d = _dev(allow_idx, np.int32)
        if cand is not None:
            cand_d, n_cand = _dev(np.append(cand, 0), np.int32), len(cand)
        return (ip_d, idx_d, bits_d, ai_d, cand_d), words, n_masks, n_cand

    def __call__(self, n, n_slices, T, seed, streams=None, seen=None, bits=None, allow_idx=None, cand=None, expect=None, null=(), **over):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        nu, ni = self.n_users, self.n_items
        cols = max(1, min(n, MAX_TOPN + 1))
        need = int(lib.wmf_sample_workspace_bytes(nu, max(1, min(n, MAX_TOPN)), max(0, min(n_slices, 256))))
        ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        items = torch.full((nu + 2, cols), -7, dtype=torch.int32, device="cuda")
        sc = torch.full((nu + 2, cols), fc.SENTINEL, dtype=torch.float32, device="cuda")
        keys = torch.full((nu + 2, cols), fc.SENTINEL, dtype=torch.float32, device="cuda")
        cnt = torch.full((nu + 2,), -7, dtype=torch.int32, device="cuda")
        (ip_d, idx_d, bits_d, ai_d, cand_d), words, n_masks, n_cand = self._filter(seen, bits, allow_idx, cand)
        st_d = None if streams is None else _dev(np.asarray(streams, dtype=np.uint64).view(np.int64))
        assert st_d is None or len(st_d) == nu
        ptr = {"users": _ptr(self.Ud), "items": _ptr(self.Id), "user_idx": _ptr(self.user_idx), "out_items": _ptr(items[1:]), "workspace": _ptr(ws)}
        for name in null:
            ptr[name] = None
        rc = lib.wmf_sample_topn(ptr["users"], ptr["items"], f, ld, bias, ptr["user_idx"], nu, ni, _ptr(ip_d), _ptr(idx_d), _ptr(bits_d),
                                 over.get("allow_words", words), over.get("n_masks", n_masks), _ptr(ai_d), _ptr(cand_d), over.get("n_cand", n_cand),
                                 n, n_slices, float(T), seed, _ptr(st_d), ptr["out_items"], _ptr(sc[1:]), _ptr(keys[1:]), _ptr(cnt[1:]),
                                 ptr["workspace"], over.get("ws_bytes", need), _stream())
        items, sc, keys, cnt, tail = items.cpu().numpy(), sc.cpu().numpy(), keys.cpu().numpy(), cnt.cpu().numpy(), ws[need:].cpu().numpy()
        assert (tail == GUARD_BYTE).all(), "the guard region past workspace_bytes was written"
        for a, fill in ((items, -7), (sc, np.float32(fc.SENTINEL)), (keys, np.float32(fc.SENTINEL)), (cnt, -7)):
            assert (a[0] == fill).all() and (a[-1] == fill).all(), "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (items == -7).all() and (sc == np.float32(fc.SENTINEL)).all() and (keys == np.float32(fc.SENTINEL)).all() and (cnt == -7).all()
            return None
        _lib.check(rc)
        return items[1:-1], sc[1:-1], keys[1:-1], cnt[1:-1]

    def logz(self, T, n_slices=0, seen=None, bits=None, allow_idx=None, cand=None, expect=None, null=(), **over):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        nu, ni = self.n_users, self.n_items
        need = int(lib.wmf_log_partition_workspace_bytes(nu, max(0, min(n_slices, 256))))
        ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        out = torch.full((nu + 2,), fc.SENTINEL, dtype=torch.float32, device="cuda")
        elig = torch.full((nu + 2,), -7, dtype=torch.int32, device="cuda")
        (ip_d, idx_d, bits_d, ai_d, cand_d), words, n_masks, n_cand = self._filter(seen, bits, allow_idx, cand)
        ptr = {"users": _ptr(self.Ud), "items": _ptr(self.Id), "user_idx": _ptr(self.user_idx), "out_logz": _ptr(out[1:]), "workspace": _ptr(ws)}
        for name in null:
            ptr[name] = None
        rc = lib.wmf_log_partition(ptr["users"], ptr["items"], f, ld, bias, ptr["user_idx"], nu, ni, _ptr(ip_d), _ptr(idx_d), _ptr(bits_d),
                                   over.get("allow_words", words), over.get("n_masks", n_masks), _ptr(ai_d), _ptr(cand_d), over.get("n_cand", n_cand),
                                   float(T), n_slices, ptr["out_logz"], _ptr(elig[1:]), ptr["workspace"], over.get("ws_bytes", need), _stream())
        out, elig, tail = out.cpu().numpy(), elig.cpu().numpy(), ws[need:].cpu().numpy()
        assert (tail == GUARD_BYTE).all(), "the guard region past workspace_bytes was written"
        assert out[0] == out[-1] == np.float32(fc.SENTINEL) and elig[0] == elig[-1] == -7
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (out == np.float32(fc.SENTINEL)).all() and (elig == -7).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return out[1:-1], elig[1:-1]


def _check_exact(got, M, users, seen, n, T, g32, what, masks=None):
    """Items, key bits, score bits, counts and padding against the reference; g32: the device's noise [rows, n_items] of the rows'
    streams; masks: bool [rows, n_items], the complement joins the seen row."""
    items, sc, keys, cnt = got
    z = sref.perturbed_exact(M[users], T, g32) + np.float32(0)       # (-0.0 is +0.0 in a key)
    want = []
    for b in range(len(users)):
        s = np.asarray([] if seen is None else seen[b], dtype=np.int64)
        if masks is not None:
            s = np.concatenate([s, np.flatnonzero(~masks[b])])
        want.append(sref.sample_row(z[b], s, n))
    want_items = rref.padded_rows(want, n, -1, np.int32)
    assert np.array_equal(items, want_items), (what, np.argwhere(items != want_items)[:5])
    assert np.array_equal(cnt, [len(w) for w in want]), what
    valid = want_items >= 0
    rows = np.repeat(np.arange(len(users)), valid.sum(axis=1))
    assert (sc[~valid] == -np.inf).all() and (keys[~valid] == -np.inf).all(), what
    assert np.array_equal(keys[valid].view(np.int32), z[rows, want_items[valid]].view(np.int32)), what
    assert np.array_equal(sc[valid].view(np.int32), M[np.asarray(users)[rows], want_items[valid]].astype(np.float32).view(np.int32)), what
    for b in range(len(users)):                                       # draw order: z descending
        assert (np.diff(keys[b, :cnt[b]]) <= 0).all(), what


def _bits(got):
    return [np.ascontiguousarray(a).view(np.int32) for a in got]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# --------------------------------------------------------------------------------------------------------------- 1. the noise
EDGES = (0, 1, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 63, U64)


def test_noise_hash_and_accuracy():
    """2^20 (seed, stream, item) triples, 16 seeds of 65536 pairs, the edges among them: k bit for bit; g within 4 * 2^-23 *
    max(1, |g64|) of the float64 value (two logf of an ulp each: 2^-23 (1 + |g|); the gate is twice that) and inside its range."""
    rng = np.random.default_rng(100)
    seeds = list(EDGES) + [int(x) for x in rng.integers(0, 2 ** 64, 10, dtype=np.uint64)]
    worst, g_lo, g_hi = 0.0, np.inf, -np.inf
    for seed in seeds:
        streams = rng.integers(0, 2 ** 64, 65536, dtype=np.uint64)
        items = rng.integers(0, 2 ** 31, 65536).astype(np.int64)
        edge_pairs = [(s, i) for s in EDGES for i in (0, 1, 2 ** 31 - 1, -1)]
        streams[:len(edge_pairs)] = [s for s, _ in edge_pairs]
        items[:len(edge_pairs)] = [i for _, i in edge_pairs]
        g, k = _noise(seed, streams, items)
        want_k = sref.noise_k(seed, streams, items)
        assert np.array_equal(k, want_k), (seed, np.flatnonzero(k != want_k)[:5])
        g64 = sref.noise_g(want_k)
        err = np.abs(g.astype(np.float64) - g64) / np.maximum(1.0, np.abs(g64))
        worst, g_lo, g_hi = max(worst, float(err.max())), min(g_lo, float(g.min())), max(g_hi, float(g.max()))
    print(f"noise: worst |g - g64| / max(1, |g64|) = {worst / 2.0 ** -23:.3f} x 2^-23, g in [{g_lo:.4f}, {g_hi:.4f}]")
    record_error("sample_noise", worst_ulp23=worst / 2.0 ** -23, g_min=g_lo, g_max=g_hi)
    assert worst <= 4 * 2.0 ** -23
    assert sref.G_MIN <= g_lo and g_hi <= sref.G_MAX
    # row_stream NULL: the pair's index
    g0, k0 = _noise(5, None, np.arange(1000))
    assert np.array_equal(k0, sref.noise_k(5, np.arange(1000), np.arange(1000)))


# ------------------------------------------------------------------------------------------------------------ 2. exact inputs
@wide
@pytest.mark.parametrize("n_items", (300, 2000, 2063))
def test_exact_table(f, bias, n_items):
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    rng = np.random.default_rng(11000 + 2 * f + bias + n_items)
    seen = _seen_rows(rng, M[users], n_items, n_items % 8)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    seed = 17 * f + n_items
    g32 = _noise_rows(seed, np.arange(N_USERS), n_items)
    for i, n in enumerate(NS):
        T = TEMPS[(i + f + bias) % 3]
        _check_exact(run(n, 0, T, seed, None, seen), M, users, seen, n, T, g32, (f, bias, n_items, n, T))
    _check_exact(run(NS[-1], 0, 1.0, seed), M, users, None, NS[-1], 1.0, g32, (f, bias, n_items, "no seen list"))


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("n", NS)
def test_every_n_at_every_temperature(n, T):
    f, bias, n_items = 5, 1, 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    seen = _seen_rows(np.random.default_rng(11100 + n), M[users], n_items, n)
    streams = np.random.default_rng(n).integers(0, 2 ** 64, N_USERS, dtype=np.uint64)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    _check_exact(run(n, 0, T, U64, streams, seen), M, users, seen, n, T, _noise_rows(U64, streams, n_items), (n, T))


@pytest.mark.parametrize("f,bias,extra", [(f, b, e) for f in (5, 64, 129, 260) for b in (0, 1) for e in (0, LD_EXTRA[f])])
def test_both_leading_dimensions(f, bias, extra):
    ld = _ld(f, extra)
    M, _ = _scores(f, bias, "exact")
    users = _user_list()
    seen = _seen_rows(np.random.default_rng(11200 + 2 * f + bias + extra), M[users], N_ITEMS, f % 8)
    run = Sample(*_host(f, "exact"), f, ld, bias, users)
    g32 = _noise_rows(3, np.arange(N_USERS), N_ITEMS)
    for n, T in ((10, 0.25), (129, 4.0)):
        _check_exact(run(n, 0, T, 3, None, seen), M, users, seen, n, T, g32, (f, bias, ld, n))


@pytest.mark.parametrize("rows", (1, 15, 16, 17, 129))
def test_batch_sizes(rows):
    """The eight seen-row patterns in turn; one user twice (positions 2 and 9) under the default streams: two lists."""
    f, bias, n_items = 5, 1, 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list(rows)
    seen = _seen_rows(np.random.default_rng(11300 + rows), M[users], n_items, rows)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    g32 = _noise_rows(rows, np.arange(rows), n_items)
    for n, T in ((129, 1.0), (1000, 0.25)):
        got = run(n, 0, T, rows, None, seen)
        _check_exact(got, M, users, seen, n, T, g32, (rows, n))
    if rows > 9:
        assert users[2] == users[9] and not np.array_equal(got[0][2], got[0][9])


@pytest.mark.parametrize("shape", ("all equal", "blocks of 17", "ascending"))
def test_tied_scores_are_ordered_by_the_noise(shape):
    """f = 1: the score is the item's value.  All equal: the list is the order of the noise alone."""
    n_items = 5000
    j = np.arange(n_items, dtype=np.int64)
    value = {"all equal": 0 * j + 3, "blocks of 17": j // 17 % 64, "ascending": j % 2048}[shape]
    Uf, If = np.ones((4, 1), dtype=np.float32), value.astype(np.float32)[:, None]
    Uf[:, 0] = [1, -1, 0, 2]
    M = ref.score_matrix_int(Uf, If, np.arange(4), j, 0)
    users = np.arange(4)
    seen = [np.arange(0), np.arange(0, n_items, 2), np.arange(n_items - 40, n_items), np.arange(100)]
    run = Sample(Uf, If, 1, _ld(1), 0, users)
    g32 = _noise_rows(77, np.arange(4), n_items)
    for n, T in ((10, 1.0), (129, 0.25), (1000, 4.0)):
        for s in (None, seen):
            got = run(n, 0, T, 77, None, s)
            _check_exact(got, M, users, s, n, T, g32, (shape, n, T, s is not None))


# ------------------------------------------------------------------------------------------------------------ 3. invariances
@pytest.mark.parametrize("f,bias", [(5, 1), (129, 0)])
def test_the_result_does_not_depend_on_the_slices_or_the_batch(f, bias):
    n_items = 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    seen = _seen_rows(np.random.default_rng(11400 + f), M[users], n_items, 4)
    streams = np.arange(N_USERS, dtype=np.uint64) * np.uint64(7919)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    limit = _constant("WMF_RECOMMEND_MAX_SLICES", "include/wmf_hip.h")
    for n, T in ((10, 1.0), (129, 0.25), (1000, 4.0)):
        first = run(n, 0, T, 9, streams, seen)
        assert _same(run(n, 0, T, 9, streams, seen), first), "two runs, the same bits"
        for n_slices in range(1, limit + 1) if n == 129 else (1, 2, 3, 7, 64, limit):
            assert _same(run(n, n_slices, T, 9, streams, seen), first), (f, bias, n, n_slices)
        for b in (0, 9, 39):                                         # a row alone, with its stream kept
            alone = Sample(*_factors(f, n_items), f, _ld(f), bias, users[b: b + 1])(n, 0, T, 9, streams[b: b + 1], seen[b: b + 1])
            assert _same(alone, [a[b: b + 1] for a in first]), (f, bias, n, b)
        # ... moved to another batch position
        perm = np.roll(np.arange(N_USERS), 5)
        moved = Sample(*_factors(f, n_items), f, _ld(f), bias, users[perm])(n, 0, T, 9, streams[perm], [seen[p] for p in perm])
        assert _same(moved, [a[perm] for a in first]), (f, bias, n, "moved")
        # the list of n is a prefix of the list of n' > n
        longer = run(min(2 * n + 3, 2000), 0, T, 9, streams, seen)
        assert all(np.array_equal(x[:, :n], y) for x, y in zip(_bits(longer[:3]), _bits(first[:3]))), (f, bias, n, "prefix")
    assert not _same(run(10, 0, 1.0, 10, streams, seen)[:1], run(10, 0, 1.0, 9, streams, seen)[:1]), "another seed, another draw"


def test_beyond_both_grid_caps():
    f, bias, n, n_slices, n_items, rows = 5, 1, 129, 256, 4200, 1100
    scan_cap = _constant("WMF_SCAN_GRID", "recmodel_amd/csrc/wmf_scan.h")
    select_cap = _constant("WMF_SAMPLE_SELECT_GRID", "recmodel_amd/csrc/wmf_sample.hip")
    waves = _constant("WMF_REC_WIDE_WAVES", "recmodel_amd/csrc/wmf_topn_wide.h")
    assert -(-rows // (16 * waves)) * n_slices > scan_cap and rows > select_cap
    M = _int_scores(f, bias, n_items)
    users = np.arange(rows) % N_USERS
    seen = [np.array([(7 * b) % n_items]) for b in range(rows)]
    streams = (np.arange(rows) % 64).astype(np.uint64)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    got = run(n, n_slices, 1.0, 4, streams, seen)
    g32 = _noise_rows(4, np.arange(64), n_items)[np.arange(rows) % 64]
    _check_exact(got, M, users, seen, n, 1.0, g32, "both caps")
    assert _same(run(n, 0, 1.0, 4, streams, seen), got)


@pytest.mark.parametrize("n", (10, 129, 1000))
def test_mask_form_list_form_and_the_complement_in_the_seen_rows(n):
    f, bias, n_items = 5, 1, 2063
    M = _int_scores(f, bias, n_items)
    users = _user_list()
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    g32 = _noise_rows(21, np.arange(N_USERS), n_items)
    for pattern in range(len(fc.PATTERNS)):
        rng = np.random.default_rng(11500 + 100 * pattern)
        seen = _seen_rows(rng, M[users], n_items, pattern)
        masks = fc.mask_rows(pattern, rng, M[users], seen, n_items)
        bits, allow_idx = fc.bits_of(pattern, masks)
        got = run(n, 0, 1.0, 21, None, seen, bits=bits, allow_idx=allow_idx)
        what = (n, fc.PATTERNS[pattern])
        assert _same(got, run(n, 0, 1.0, 21, None, _with_complement(seen, masks))), what
        _check_exact(got, M, users, seen, n, 1.0, g32, what, masks)
        if allow_idx is None and masks[0].any():                     # one mask for every row: the list form of it, keyed by the real id
            assert _same(got, run(n, 0, 1.0, 21, None, seen, cand=np.flatnonzero(masks[0]))), what


def test_one_user_under_two_masks_and_under_two_streams():
    f, bias, n_items, n = 5, 1, 2063, 129
    M = _int_scores(f, bias, n_items)
    users = np.array([3, 3, 3, 3])
    rng = np.random.default_rng(11600)
    G = np.stack([fc.mask_row(p, rng, M[3], [], n_items) for p in (6, 9)])
    allow_idx = np.array([0, 1, 0, -1])
    streams = np.array([5, 5, 6, 5], dtype=np.uint64)
    run = Sample(*_factors(f, n_items), f, _ld(f), bias, users)
    got = run(n, 0, 1.0, 8, streams, None, bits=fc.pack(G), allow_idx=allow_idx)
    masks = np.where(allow_idx[:, None] < 0, True, G[allow_idx])
    _check_exact(got, M, users, None, n, 1.0, _noise_rows(8, streams, n_items), "two masks, two streams", masks)
    assert not np.array_equal(got[0][0], got[0][1]) and not np.array_equal(got[0][0], got[0][2])
    same = Sample(*_factors(f, n_items), f, _ld(f), bias, users)(n, 0, 1.0, 8, np.array([5, 5, 5, 5], dtype=np.uint64))
    assert all(np.array_equal(a[0], a[b]) for a in _bits(same) for b in range(4)), "one user, one stream, one list"


# ------------------------------------------------------------------------------------------------------- 4. temperature zero
@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
@pytest.mark.parametrize("cls", ("exact", "rounded"))
def test_temperature_zero_is_the_wide_top_n(f, bias, cls):
    users = _user_list()
    S, _ = _scores(f, bias, cls)
    seen = _seen_rows(np.random.default_rng(11700 + f), S[users], N_ITEMS, 2)
    mask = fc.mask_row(9, np.random.default_rng(1), None, None, N_ITEMS)
    new, old = Sample(*_host(f, cls), f, _ld(f), bias, users), Wide(*_host(f, cls), f, _ld(f), bias, users)
    cls_name = {5: "4, 4", 64: "4, 4", 129: "9, 2", 260: "17, 1"}[f]
    for seed in (0, 123456789):
        for n in (1, 10, 129):
            for form, tag in (({}, ""), ({"bits": fc.pack(mask)}, "mask_"), ({"cand": np.flatnonzero(mask)}, "list_")):
                got = {}
                names = _launched(lambda: got.update(out=new(n, 0, 0.0, seed, None, seen, **form)))
                assert names == {f"sample_scan_{tag}kernel<{cls_name}, 4>", "sample_select_kernel"}, names
                items, sc, keys, cnt = got["out"]
                assert fc.same_bits((items, sc, cnt), old(n, 0, seen, **form)), (f, bias, cls, seed, n, tag)
                assert np.array_equal(keys.view(np.int32), sc.view(np.int32))


# ------------------------------------------------------------------------------------------------------------ 5. model scores
@wide
def test_out_scores_are_the_scan_s_own_bits(f, bias):
    """Gaussian factors: the scores of the picks equal, bit for bit, what wmf_recommend_topn_wide returns for the same ids -- asked
    for through the list form of each row's sorted picks."""
    n_items, n = 2063, 129
    Uf, If = _factors(f, n_items, "rounded")
    users = _user_list()[:12]
    run = Sample(Uf, If, f, _ld(f), bias, users)
    items, sc, keys, cnt = run(n, 0, 1.0, 31)
    assert (cnt == n).all() and (np.diff(keys, axis=1) <= 0).all()
    for b, u in enumerate(users):
        picks = np.sort(items[b])
        assert len(np.unique(picks)) == n
        w_items, w_sc, _ = Wide(Uf, If, f, _ld(f), bias, users[b: b + 1])(n, 0, cand=picks)
        by_id = dict(zip(w_items[0].tolist(), w_sc[0].view(np.int32).tolist()))
        assert [by_id[i] for i in items[b].tolist()] == sc[b].view(np.int32).tolist(), (f, bias, b)
        g = _noise_rows(31, [b], n_items)[0]
        assert np.array_equal(np.float32(1.0) * g[items[b]] + sc[b], keys[b]), "z = fmaf(1, g, score): one rounding of the sum"


# -------------------------------------------------------------------------------------------------- 6. chi-square on the device
@pytest.mark.parametrize("temperature", CHI_TEMPERATURES)
def test_chi_square_on_the_device(temperature):
    """f = 1, the user factor 1, the item factors the scores; user 0 repeated under streams 0 .. 8191."""
    Uf, If = np.ones((1, 1), dtype=np.float32), CHI_SCORES.astype(np.float32)[:, None]
    run = Sample(Uf, If, 1, _ld(1), 0, np.zeros(CHI_STREAMS, dtype=np.int64))
    items, sc, keys, cnt = run(2, 0, temperature, CHI_SEED)
    assert (cnt == 2).all() and np.array_equal(sc, CHI_SCORES.astype(np.float32)[items])
    first, second, cells = chi_square_gate(items, temperature)
    print(f"T = {temperature}: first picks {first:.1f} at 7 degrees of freedom, pairs {second:.1f} over {cells} cells")
    record_error(f"sample_chi_square[{temperature}]", first=first, pairs=second, cells=cells)


# ------------------------------------------------------------------------------------------------------- 7. wmf_log_partition
def _logz_gate(L64, n_elig, B, T):
    return B / T + 4 * 2.0 ** -23 * (2 + math.log(n_elig)) + 2.0 ** -23 * abs(L64)


def _check_logz(got, S, Bd, users, T32, seen, masks, what):
    """out_logz within the gate of the float64 log-sum-exp of the float64 scores, the eligible count exactly.  Returns the worst
    error / gate."""
    L, elig = got
    T, worst = float(T32), 0.0
    for b, u in enumerate(users):
        keep = np.ones(S.shape[1], dtype=bool)
        if seen is not None:
            keep[np.asarray(seen[b], dtype=np.int64)] = False
        if masks is not None:
            keep &= masks[b]
        assert elig[b] == keep.sum(), (what, b)
        if not keep.any():
            assert L[b] == -np.inf, (what, b)
            continue
        L64 = sref.logsumexp64(S[u, keep] / T)
        ratio = abs(float(L[b]) - L64) / _logz_gate(L64, int(keep.sum()), float(Bd[u, keep].max()), T)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, b, float(L[b]), L64, ratio)
    return worst


@wide
@pytest.mark.parametrize("T", (0.1, 1.0, 10.0))
def test_log_partition(f, bias, T):
    """Gaussian factors; no filter, the seen rows (pattern 1 leaves nothing eligible), the mask form, the list form; two runs
    bit-identical; every slice count within the gate."""
    T32 = np.float32(T)
    users = _user_list()
    S, Bd = _scores(f, bias, "rounded")
    rng = np.random.default_rng(11800 + 2 * f + bias)
    seen = _seen_rows(rng, S[users], N_ITEMS, 0)
    assert any(len(s) == N_ITEMS for s in seen)
    run = Sample(*_host(f, "rounded"), f, _ld(f), bias, users)
    worst = _check_logz(run.logz(T32), S, Bd, users, T32, None, None, (f, bias, T, "plain"))
    first = run.logz(T32, 0, seen)
    worst = max(worst, _check_logz(first, S, Bd, users, T32, seen, None, (f, bias, T, "seen")))
    again = run.logz(T32, 0, seen)
    assert np.array_equal(first[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(first[1], again[1])
    for n_slices in (1, 2, 3, 5, 19):
        worst = max(worst, _check_logz(run.logz(T32, n_slices, seen), S, Bd, users, T32, seen, None, (f, bias, T, n_slices)))
    for pattern in (1, 4, 6, 9, 11):
        masks = fc.mask_rows(pattern, rng, S[users], seen, N_ITEMS)
        bits, allow_idx = fc.bits_of(pattern, masks)
        got = run.logz(T32, 0, seen, bits=bits, allow_idx=allow_idx)
        worst = max(worst, _check_logz(got, S, Bd, users, T32, seen, masks, (f, bias, T, fc.PATTERNS[pattern])))
        if allow_idx is None and masks[0].any():
            by_list = run.logz(T32, 0, seen, cand=np.flatnonzero(masks[0]))
            worst = max(worst, _check_logz(by_list, S, Bd, users, T32, seen, masks, (f, bias, T, fc.PATTERNS[pattern], "list")))
            assert np.array_equal(by_list[1], got[1])
    print(f"log_partition f={f} bias={bias} T={T}: worst error / gate = {worst:.4f}")
    record_error(f"log_partition[{f}-{bias}-{T}]", worst_over_gate=worst)


def test_log_partition_kernels_and_many_rows():
    """Past the merge's grid cap; the kernels' names."""
    f, bias, rows = 5, 1, 4200
    cap = _constant("WMF_LOGZ_MERGE_GRID", "recmodel_amd/csrc/wmf_sample.hip")
    assert rows > 4 * cap
    users = np.arange(rows) % N_USERS
    S, Bd = _scores(f, bias, "rounded")
    run = Sample(*_host(f, "rounded"), f, _ld(f), bias, users)
    got = {}
    names = _launched(lambda: got.update(out=run.logz(np.float32(1.0), 0)))
    assert names == {"logz_scan_kernel<4, 4, 4>", "logz_merge_kernel"}
    L, elig = got["out"]
    _check_logz((L[:N_USERS], elig[:N_USERS]), S, Bd, users[:N_USERS], np.float32(1.0), None, None, "many rows")
    assert all(np.array_equal(L[b::N_USERS].view(np.int32), np.full(len(L[b::N_USERS]), L[b].view(np.int32))) for b in range(N_USERS))


# -------------------------------------------------------------------------------------------------------------- 8. WMF_EINVAL
def test_refusals_come_before_any_launch():
    _lib = _api()[0]
    f, bias = 5, 1
    run = Sample(*_host(f, "exact"), f, _ld(f), bias, _user_list())
    bits, cand = fc.pack(fc.mask_row(6, None, None, None, N_ITEMS)), np.arange(0, N_ITEMS, 3)
    E = _lib.WMF_EINVAL
    lib = _api()[1]

    def refused():
        for bad_T in (-1.0, float("nan"), float("inf"), -float("inf")):
            run(129, 0, bad_T, 1, expect=E)
            run.logz(bad_T, expect=E)
        run.logz(0.0, expect=E)
        run(0, 0, 1.0, 1, expect=E)
        run(MAX_TOPN + 1, 0, 1.0, 1, expect=E)
        for call in (lambda **k: run(129, k.pop("n_slices", 0), 1.0, 1, **k), lambda **k: run.logz(1.0, k.pop("n_slices", 0), **k)):
            call(bits=bits, cand=cand, expect=E)
            call(bits=bits, n_masks=0, expect=E)
            call(bits=bits, allow_words=9, expect=E)
            call(allow_idx=np.zeros(N_USERS), expect=E)
            call(cand=cand, n_cand=0, expect=E)
            call(cand=cand, n_cand=N_ITEMS + 1, expect=E)
            call(n_slices=-1, expect=E)
            call(n_slices=257, expect=E)
            for name in ("users", "items", "user_idx", "workspace"):
                call(null=(name,), expect=E)
        run(129, 0, 1.0, 1, null=("out_items",), expect=E)
        run.logz(1.0, null=("out_logz",), expect=E)
        for form in ({}, {"bits": bits}, {"cand": cand}):
            run(129, 0, 1.0, 1, ws_bytes=int(lib.wmf_sample_workspace_bytes(N_USERS, 129, 0)) - 1, expect=E, **form)
            run.logz(1.0, 0, ws_bytes=int(lib.wmf_log_partition_workspace_bytes(N_USERS, 0)) - 1, expect=E, **form)
    assert _launched(refused) == set()
