"""wmf_rerank_mmr and wmf_intra_list_similarity through the C ABI, per element, against tests/mmr_ref.py.

EXACT inputs (small-integer factors with the dot product, rows whose squared norm is a power of four with the cosine, integer
relevances, lambda a multiple of 1/4): every operation is exact in float32, the reference's pick sequence is forced, and items,
score bits, marginal bits and counts are compared for equality.  ROUNDED inputs (Gaussian factors and scores): near-ties make the
greedy path sensitive to rounding, so every step of every row is held to the step-wise condition of mmr_ref.step_shortfalls
instead -- given the device's own prefix, the float64 v of its pick is within 2 E of the best remaining one, E = mmr_ref.v_bound
(derived in DESIGN.md section 5, not taken from any output).  The largest shortfall observed on an MI355X, as a multiple of E, is
recorded per shape in profiles/r21_mmr.json.  Every call keeps a sentinel row on either side of each output."""
import functools

import numpy as np
import pytest
import torch

import mmr_ref as mref
import serving_ref as ref
from conftest import record_error
from scan_cases import _api, _dev, _ld

pytestmark = pytest.mark.gpu

N_ITEMS = 500
SENT_I, SENT_F = -7, np.float32(-12345.0)
# the widths of the issue, with and without the bias column, at both leading dimensions the serving tests use (scan_cases.LD_EXTRA)
SHAPES = [(f, b, e) for f, extras in ((1, (0,)), (5, (0, 4)), (64, (0, 4)), (129, (0, 4)), (260, (0, 12))) for b in (0, 1) for e in extras
          if f >= 2 or not b]
shape = pytest.mark.parametrize("f,bias,extra", SHAPES, ids=[f"f{f}-b{b}" + (f"-ld+{e}" if e else "") for f, b, e in SHAPES])
metric = pytest.mark.parametrize("cosine", (False, True), ids=("dot", "cosine"))
POOLS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096)


# ------------------------------------------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=None)
def _items(f, bias, cosine, cls="exact"):
    """The item factors of a class, unpadded; item 0 and item N_ITEMS - 1 are ordinary rows.  Computed once, never written."""
    if cls == "rounded":
        F = ref.rounded_factors(N_ITEMS, f, 10 * f + 7)
    else:
        F = mref.pow4_items(N_ITEMS, f, bias, 10 * f + 5) if cosine else mref.exact_items(N_ITEMS, f, 10 * f + 5)
    F.setflags(write=False)
    return F


def _resident(f, ld):
    return int(_api()[1].wmf_rerank_mmr_resident_pool(f, ld))


class Mmr:
    """wmf_rerank_mmr on one item matrix: the device inverse norms are wmf_row_inv_norms' own."""

    def __init__(self, F, f, ld, bias, cosine):
        _lib, lib, _ptr, _stream = _api()
        self.F, self.args, self.cosine = F, (f, ld, bias), cosine
        self.Id = _dev(ref.padded(F, ld))
        self.inv = None
        if cosine:
            self.inv = torch.empty(len(F), dtype=torch.float32, device="cuda")
            _lib.check(lib.wmf_row_inv_norms(_ptr(self.Id), len(F), f, ld, bias, _ptr(self.inv), _stream()))

    def __call__(self, ids, r, count, lam, topn, expect=None, null=(), **over):
        """ids, r: [B, pool]; count: int [B] or None (NULL).  Returns (items, scores, marginal, counts) of the B rows."""
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        ids, r = np.atleast_2d(ids), np.atleast_2d(r)
        B, pool = ids.shape
        cols = max(1, min(int(topn), 129))
        ids_d, r_d = _dev(ids, np.int32), _dev(r, np.float32)
        cnt_d = None if count is None else _dev(count, np.int32)
        items = torch.full((B + 2, cols), SENT_I, dtype=torch.int32, device="cuda")          # a sentinel row on either side
        sc = torch.full((B + 2, cols), float(SENT_F), dtype=torch.float32, device="cuda")
        mg = torch.full((B + 2, cols), float(SENT_F), dtype=torch.float32, device="cuda")
        cnt = torch.full((B + 2,), SENT_I, dtype=torch.int32, device="cuda")
        ptr = {"items": _ptr(self.Id), "pool_items": _ptr(ids_d), "pool_scores": _ptr(r_d), "out_items": _ptr(items[1:])}
        for name in null:
            ptr[name] = None
        rc = lib.wmf_rerank_mmr(ptr["items"], over.get("n_items", len(self.F)), over.get("f", f), over.get("ld", ld), bias, _ptr(self.inv),
                                ptr["pool_items"], ptr["pool_scores"], _ptr(cnt_d), over.get("n_rows", B), over.get("pool", pool), lam, topn,
                                ptr["out_items"], _ptr(sc[1:]), _ptr(mg[1:]), _ptr(cnt[1:]), _stream())
        items, sc, mg, cnt = items.cpu().numpy(), sc.cpu().numpy(), mg.cpu().numpy(), cnt.cpu().numpy()
        for a, fill in ((items, SENT_I), (sc, SENT_F), (mg, SENT_F), (cnt, SENT_I)):
            assert (a[0] == fill).all() and (a[-1] == fill).all(), "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (items == SENT_I).all() and (sc == SENT_F).all() and (mg == SENT_F).all() and (cnt == SENT_I).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return items[1:-1], sc[1:-1], mg[1:-1], cnt[1:-1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_exact(m, got, ids, r, count, lam, topn, what):
    """Items, score bits, marginal bits, counts and padding of every row against the float32 form of the reference."""
    items, sc, mg, cnt = got
    f, ld, bias = m.args
    for b in range(len(ids)):
        c = ids.shape[1] if count is None else int(count[b])
        sims = mref.RowSims(m.F, bias, ids[b, :c], m.cosine, "f32")
        picks, values = mref.mmr_greedy(r[b, :c], sims.column, lam, topn)
        wi, ws, wm = mref.padded_outputs(ids[b, :c], r[b, :c], picks, values, topn)
        assert cnt[b] == min(topn, c), (what, b)
        assert np.array_equal(items[b], wi), (what, b, items[b][:8], wi[:8])
        assert np.array_equal(_bits(sc[b]), _bits(ws)), (what, b)
        assert np.array_equal(_bits(mg[b]), _bits(wm)), (what, b, mg[b][:8], wm[:8])


def _exact_rows(rng, pool, big):
    """(ids, r, count) of one batch, one row per pattern: 0 random relevances with item 0, the last item, a duplicated id and the
    zero-norm item (N_ITEMS // 2 of pow4_items, and a zero row of exact_items) among the candidates; 1 no candidates; 2 one
    candidate; 3 a count somewhere inside; 4 all relevances equal; 5 all candidates identical; 6 block ties in v: two relevance
    levels over three distinct items, a -0.0 relevance among them.  Large pools keep patterns 0, 3 and 6."""
    patterns = (0, 3, 6) if big else (0, 1, 2, 3, 4, 5, 6)
    ids = rng.integers(0, N_ITEMS, (len(patterns), pool))
    r = rng.integers(-6, 7, (len(patterns), pool)).astype(np.float32)
    count = np.full(len(patterns), pool)
    for b, p in enumerate(patterns):
        if p == 0:
            where = rng.choice(pool, min(pool, 5), replace=False)
            ids[b, where] = np.array([0, N_ITEMS - 1, N_ITEMS // 2, 42, 42])[:len(where)]
        elif p == 1:
            count[b] = 0
        elif p == 2:
            count[b] = 1
        elif p == 3:
            count[b] = int(rng.integers(1, pool + 1))
        elif p == 4:
            r[b] = 3
        elif p == 5:
            ids[b] = ids[b, 0]
        else:
            ids[b] = rng.choice(np.array([3, 11, N_ITEMS - 2]), pool)
            r[b] = rng.choice(np.array([2.0, -0.0], dtype=np.float32), pool)
    return ids, r, count


def _topns(c):
    return sorted({t for t in (1, 2, c - 1, c, c + 1, 128) if 1 <= t <= 128})


# ---------------------------------------------------------------------------------------------- 1. exact, bit for bit
@shape
@metric
def test_exact_inputs_match_the_reference_bit_for_bit(f, bias, extra, cosine):
    ld = _ld(f, extra)
    m = Mmr(_items(f, bias, cosine), f, ld, bias, cosine)
    res = _resident(f, ld)
    pools = sorted(set(POOLS) | {p for p in (res - 1, res, res + 1, res + 2) if 1 <= p <= 4096})
    rng = np.random.default_rng(1000 * f + 10 * bias + extra + cosine)
    turn = 0
    for pool in pools:
        big = pool >= 1000
        topns = _topns(pool) if not big else (1, 128)
        if pool in (res, res + 1) and not big:
            topns = sorted(set(topns) | {128})
        for topn in topns:
            lam = mref.LAMBDAS[turn % len(mref.LAMBDAS)]
            turn += 1
            ids, r, count = _exact_rows(rng, pool, big)
            null_count = pool in (17, 257) and topn == 2          # pool_count == NULL: every row is a full row
            got = m(ids, r, None if null_count else count, lam, topn)
            _check_exact(m, got, ids, r, None if null_count else count, lam, topn, (pool, topn, lam))


@metric
def test_every_lambda_at_the_routing_threshold(cosine):
    """All five lambdas on both sides of wmf_rerank_mmr_resident_pool at k = 128 + bias."""
    f, bias = 129, 1
    ld = _ld(f)
    m = Mmr(_items(f, bias, cosine), f, ld, bias, cosine)
    res = _resident(f, ld)
    rng = np.random.default_rng(77 + cosine)
    for pool in (res, res + 1):
        ids, r, count = _exact_rows(rng, pool, False)
        for lam in mref.LAMBDAS:
            _check_exact(m, m(ids, r, count, lam, 20), ids, r, count, lam, 20, (pool, lam))


# ---------------------------------------------------------------------------------------------------- 2. invariants
def _launched(run):
    _lib, lib, _ptr, _stream = _api()
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        lib.wmf_profile_enable(0)
    names = {name for name, *_ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return out, names


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
@pytest.mark.parametrize("cls", ("exact", "rounded"))
@metric
def test_resident_and_streaming_kernels_give_the_same_bits(f, bias, cls, cosine):
    """The same candidates once in a pool the resident kernel takes and once, padded, in one it does not: which kernel ran is read
    from the profile table, and the four outputs are the same bits."""
    ld = _ld(f)
    m = Mmr(_items(f, bias, cosine, cls), f, ld, bias, cosine)
    res = _resident(f, ld)
    assert res < 4096
    np_ = (ld // 4 + 15) // 16
    rng = np.random.default_rng(5 + f)
    c = min(res, 300)
    ids = rng.integers(0, N_ITEMS, (5, 4096))
    r = (rng.integers(-6, 7, (5, 4096)) if cls == "exact" else rng.standard_normal((5, 4096))).astype(np.float32)
    count = np.array([c, c - 1, 1, 0, c // 2])
    lam = 0.5 if cls == "exact" else 0.37
    small, names_small = _launched(lambda: m(ids[:, :c], r[:, :c], count, lam, 40))
    large, names_large = _launched(lambda: m(ids, r, count, lam, 40))
    assert f"mmr_kernel<{np_}, true>" in names_small and not any("false" in n for n in names_small if n.startswith("mmr_kernel")), names_small
    assert f"mmr_kernel<{np_}, false>" in names_large and not any("true" in n for n in names_large if n.startswith("mmr_kernel")), names_large
    assert _same(small, large)


@metric
def test_a_row_depends_on_nothing_but_the_row(cosine):
    """Two runs, a row alone, and the same row at another batch position; 1030 rows of a 17-candidate pool run past the grid cap."""
    f, bias = 129, 1
    ld = _ld(f)
    m = Mmr(_items(f, bias, cosine, "rounded"), f, ld, bias, cosine)
    rng = np.random.default_rng(9)
    for pool in (200, 700):                                         # the resident kernel, the streaming kernel
        ids = rng.integers(0, N_ITEMS, (6, pool))
        r = rng.standard_normal((6, pool)).astype(np.float32)
        count = np.array([pool, pool - 3, 17, 1, pool, 0])
        first = m(ids, r, count, 0.6, 30)
        assert _same(first, m(ids, r, count, 0.6, 30))
        alone = m(ids[4:5], r[4:5], count[4:5], 0.6, 30)
        assert _same([a[4:5] for a in first], alone)
        order = np.array([4, 0, 5, 1, 3, 2])
        moved = m(ids[order], r[order], count[order], 0.6, 30)
        assert _same([a[order] for a in first], moved)
    ids = rng.integers(0, N_ITEMS, (1030, 17))
    r = rng.standard_normal((1030, 17)).astype(np.float32)
    ids[1029], r[1029] = ids[3], r[3]                              # the same row in the first and in the second trip of a workgroup
    count = rng.integers(0, 18, 1030)
    count[1029] = count[3] = 17
    got = m(ids, r, count, 0.5, 17)
    assert np.array_equal(got[3], np.minimum(17, count))
    assert _same([a[3:4] for a in got], [a[1029:1030] for a in got])
    for b in (0, 1023, 1024, 1029):                                 # rows of both trips against the step-wise condition
        c = int(count[b])
        assert set(got[0][b, :c]) <= set(ids[b, :c]) and (got[0][b, c:] == -1).all()
        pos = _positions(ids[b, :c], r[b, :c], got[0][b, :c], got[1][b, :c])
        for short, e in mref.step_shortfalls(m.F, bias, ids[b, :c], r[b, :c], pos, 0.5, cosine):
            assert short <= 2 * e


def test_every_refusal_leaves_the_outputs_untouched():
    f, bias = 64, 0
    ld = _ld(f)
    m = Mmr(_items(f, bias, True), f, ld, bias, True)
    ids = np.random.default_rng(3).integers(0, N_ITEMS, (4, 32))
    r = np.ones((4, 32), dtype=np.float32)
    E = _api()[0].WMF_EINVAL
    for lam in (-0.001, 1.001, float("nan"), float("inf")):
        m(ids, r, None, lam, 10, expect=E)
    for topn in (0, -1, 129):
        m(ids, r, None, 0.5, topn, expect=E)
    for over in (dict(pool=0), dict(pool=4097), dict(n_rows=0), dict(n_items=0), dict(f=0), dict(ld=ld + 1), dict(ld=f - 4), dict(ld=276)):
        m(ids, r, None, 0.5, 10, expect=E, **over)
    for name in ("items", "pool_items", "pool_scores", "out_items"):
        m(ids, r, None, 0.5, 10, expect=E, null=(name,))
    assert m(ids, r, None, 0.5, 10)[3].tolist() == [10, 10, 10, 10]   # and the same buffers are served once the arguments are right


def _positions(ids, r, out_items, out_scores):
    """The pool positions of a row's picks, from the ids and score bits it returned (a duplicated id with the same score is the
    same candidate as far as v goes: the lower free position is taken, as the kernel's order does)."""
    free = np.ones(len(ids), dtype=bool)
    pos = []
    for item, s in zip(out_items, out_scores):
        hit = np.flatnonzero(free & (ids == item) & (_bits(r) == _bits(np.float32(s))))
        assert len(hit), "a pick that is no remaining candidate"
        pos.append(int(hit[0]))
        free[hit[0]] = False
    return np.array(pos, dtype=np.int64)


def test_scores_are_the_bits_of_the_pool_and_lambda_one_is_the_prefix_of_the_wide_top_n():
    """wmf_recommend_topn_wide writes the pool, wmf_rerank_mmr reads those very buffers: with lambda = 1 the result is the pool's
    prefix, items and score bits, at every count the seen lists leave."""
    _lib, lib, _ptr, _stream = _api()
    f, bias, pool, topn, nu = 129, 1, 200, 50, 12
    ld = _ld(f)
    Uf, If = ref.rounded_factors(nu, f, 1), _items(f, bias, False, "rounded")
    Ud, m = _dev(ref.padded(Uf, ld)), Mmr(If, f, ld, bias, True)
    seen = [np.arange(N_ITEMS) if b == 1 else np.delete(np.arange(N_ITEMS), [5, 77, 300]) if b == 2 else np.arange(0, N_ITEMS, 3 + b) for b in range(nu)]
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])])
    ip_d, idx_d, uid = _dev(indptr, np.int64), _dev(np.concatenate(seen), np.int32), _dev(np.arange(nu), np.int32)
    need = int(lib.wmf_recommend_wide_workspace_bytes(nu, pool, 0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p_items = torch.empty(nu, pool, dtype=torch.int32, device="cuda")
    p_scores = torch.empty(nu, pool, dtype=torch.float32, device="cuda")
    p_count = torch.empty(nu, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_recommend_topn_wide(_ptr(Ud), _ptr(m.Id), f, ld, bias, _ptr(uid), nu, N_ITEMS, _ptr(ip_d), _ptr(idx_d), None, 0, 0, None,
                                           None, 0, pool, 0, _ptr(p_items), _ptr(p_scores), _ptr(p_count), _ptr(ws), need, _stream()))
    out_i = torch.full((nu, topn), SENT_I, dtype=torch.int32, device="cuda")
    out_s = torch.full((nu, topn), float(SENT_F), dtype=torch.float32, device="cuda")
    out_c = torch.full((nu,), SENT_I, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_rerank_mmr(_ptr(m.Id), N_ITEMS, f, ld, bias, _ptr(m.inv), _ptr(p_items), _ptr(p_scores), _ptr(p_count), nu, pool, 1.0,
                                  topn, _ptr(out_i), _ptr(out_s), None, _ptr(out_c), _stream()))
    pi, ps, pc = p_items.cpu().numpy(), p_scores.cpu().numpy(), p_count.cpu().numpy()
    assert pc[1] == 0 and pc[2] == 3 and pc.max() == pool
    want_c = np.minimum(pc, topn)
    assert np.array_equal(out_c.cpu().numpy(), want_c)
    keep = np.arange(topn)[None, :] < want_c[:, None]
    assert np.array_equal(out_i.cpu().numpy(), np.where(keep, pi[:, :topn], -1))
    assert np.array_equal(_bits(out_s.cpu().numpy()), _bits(np.where(keep, ps[:, :topn], -np.inf)))


# ------------------------------------------------------------------------------------------- 3. Gaussian factors and scores
@pytest.mark.parametrize("f,bias", [(5, 0), (5, 1), (64, 0), (64, 1), (129, 0), (129, 1), (260, 0), (260, 1)])
@metric
def test_gaussian_inputs_every_step_of_every_row_is_within_the_bound(f, bias, cosine):
    ld = _ld(f)
    m = Mmr(_items(f, bias, cosine, "rounded"), f, ld, bias, cosine)
    res = _resident(f, ld)
    rng = np.random.default_rng(31 * f + bias)
    worst = 0.0
    for pool in (min(100, res), min(res + 1, 4096), 400):           # resident, the first streaming pool, streaming
        ids = rng.integers(0, N_ITEMS, (6, pool))
        r = rng.standard_normal((6, pool)).astype(np.float32)
        count = np.array([pool, pool, pool - 1, max(1, pool // 2), 2, 1])
        for lam, topn in ((0.3, 20), (0.7, 20), (0.0, 5), (1.0, 5)):
            items, sc, mg, cnt = m(ids, r, count, lam, topn)
            for b in range(6):
                c, k = int(count[b]), min(topn, int(count[b]))
                assert cnt[b] == k and (items[b, k:] == -1).all() and (sc[b, k:] == -np.inf).all() and (mg[b, k:] == -np.inf).all()
                pos = _positions(ids[b, :c], r[b, :c], items[b, :k], sc[b, :k])
                steps = mref.step_shortfalls(m.F, bias, ids[b, :c], r[b, :c], pos, lam, cosine)
                assert len(steps) == k
                for t, (short, e) in enumerate(steps):
                    print(f"f={f} bias={bias} cosine={cosine} pool={pool} lam={lam} row={b} step={t}: shortfall {short:.3e}, E {e:.3e}")
                    assert short <= 2 * e, (pool, lam, b, t, short, e)
                    worst = max(worst, short / e if e > 0 else 0.0)
    record_error(f"mmr_step_shortfall_over_E[f{f}-b{bias}-{'cosine' if cosine else 'dot'}]", worst=worst)


# ------------------------------------------------------------------------------------------------ 4. intra-list similarity
class Ils:
    def __init__(self, m):
        self.m = m

    def __call__(self, lists, count, expect=None, **over):
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.m.args
        lists = np.atleast_2d(lists)
        B, width = lists.shape
        l_d = _dev(lists, np.int32)
        c_d = None if count is None else _dev(count, np.int32)
        mean = torch.full((B + 2,), float(SENT_F), dtype=torch.float32, device="cuda")
        top = torch.full((B + 2,), float(SENT_F), dtype=torch.float32, device="cuda")
        rc = lib.wmf_intra_list_similarity(_ptr(self.m.Id), len(self.m.F), f, over.get("ld", ld), bias, _ptr(self.m.inv), _ptr(l_d), _ptr(c_d),
                                           over.get("n_rows", B), over.get("width", width), _ptr(mean[1:]), _ptr(top[1:]), _stream())
        mean, top = mean.cpu().numpy(), top.cpu().numpy()
        assert mean[0] == mean[-1] == top[0] == top[-1] == SENT_F, "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect and (mean == SENT_F).all() and (top == SENT_F).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return mean[1:-1], top[1:-1]


COUNTS = np.array([0, 1, 2, 3, 128, 77, 16, 17])


@shape
@metric
def test_intra_list_similarity_exact_bit_for_bit(f, bias, extra, cosine):
    ld = _ld(f, extra)
    m = Mmr(_items(f, bias, cosine), f, ld, bias, cosine)
    rng = np.random.default_rng(f + 3)
    lists = rng.integers(0, N_ITEMS, (len(COUNTS), 128))
    lists[4, :4] = (0, N_ITEMS - 1, N_ITEMS // 2, 0)                # the first and the last item, the zero-norm item, an id twice
    mean, top = Ils(m)(lists, COUNTS)
    for b, n in enumerate(COUNTS):
        wm, wt = mref.ils_ref(mref.RowSims(m.F, bias, lists[b, :n], cosine, "f32"), int(n))
        assert _bits(mean[b]) == _bits(wm) and _bits(top[b]) == _bits(wt), (b, n, mean[b], wm, top[b], wt)
    mean3, top3 = Ils(m)(lists[:, :3], None)                       # list_count == NULL: every row is full
    for b in range(len(COUNTS)):
        wm, wt = mref.ils_ref(mref.RowSims(m.F, bias, lists[b, :3], cosine, "f32"), 3)
        assert _bits(mean3[b]) == _bits(wm) and _bits(top3[b]) == _bits(wt)
    E = _api()[0].WMF_EINVAL
    for over in (dict(width=0), dict(width=129), dict(n_rows=0), dict(ld=ld + 1)):
        Ils(m)(lists, COUNTS, expect=E, **over)


@pytest.mark.parametrize("f,bias", [(5, 1), (64, 0), (129, 1), (260, 0)])
@metric
def test_intra_list_similarity_gaussian_within_the_bound(f, bias, cosine):
    ld = _ld(f)
    m = Mmr(_items(f, bias, cosine, "rounded"), f, ld, bias, cosine)
    lists = np.random.default_rng(f).integers(0, N_ITEMS, (len(COUNTS), 128))
    mean, top = Ils(m)(lists, COUNTS)
    again = Ils(m)(lists, COUNTS)
    assert np.array_equal(_bits(mean), _bits(again[0])) and np.array_equal(_bits(top), _bits(again[1]))
    for b, n in enumerate(COUNTS):
        if n < 2:
            assert mean[b] == 0 and top[b] == -np.inf
            continue
        m64, bm, t64, bt = mref.ils_bounds(m.F, bias, lists[b, :n], cosine)
        print(f"f={f} bias={bias} cosine={cosine} n={n}: mean error {abs(float(mean[b]) - m64):.3e} of {bm:.3e}, max error {abs(float(top[b]) - t64):.3e} of {bt:.3e}")
        assert abs(float(mean[b]) - m64) <= bm and abs(float(top[b]) - t64) <= bt
