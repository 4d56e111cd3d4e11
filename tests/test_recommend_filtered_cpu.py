"""The catalogue filters without a GPU: the reference route of tests/filter_cases.py against a brute-force top-n, the case table held
to account (a case that silently filters nothing or everything would pass without testing anything), the bit packing, the argument
checks of the Python layer, and the two new symbols in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import filter_cases as fc
from conftest import ROOT
from scan_cases import N_ITEMS, N_USERS

TOPNS = (1, 10, 128)
WIDTHS = ((5, 1), (64, 0))
# what a pattern's mask of the N_ITEMS-item catalogue holds, per row: (fewest, most) items
MASK_SIZE = {"everything": (300, 300), "nothing": (0, 0), "item 0": (1, 1), "last item": (1, 1), "one tile": (12, 16),
             "all but one tile": (284, 288), "every other": (150, 150), "word edges": (4, 4), "without the 50 best": (250, 300),
             "random 30%": (50, 130), "random 1%": (0, 12), "dead bits set": (300, 300)}


@pytest.mark.parametrize("f,bias", WIDTHS)
def test_reference_route_is_the_brute_force_top_n(f, bias):
    from scan_cases import _scores
    M, _ = _scores(f, bias, "exact")
    for pattern in range(len(fc.PATTERNS)):
        users, seen, masks = fc.case_rows(f, bias, "exact", pattern)
        for topn in TOPNS:
            for b, u in enumerate(users):
                want = fc.brute_force(M[u], seen[b], masks[b], topn)
                assert np.array_equal(fc.filtered_ref(M[u], seen[b], masks[b], topn), want), (fc.PATTERNS[pattern], topn, b)


@pytest.mark.parametrize("cls", ("exact", "rounded"))
@pytest.mark.parametrize("f,bias", WIDTHS)
def test_the_case_table_filters_what_it_is_meant_to(f, bias, cls):
    assert set(MASK_SIZE) == set(fc.PATTERNS) and len(fc.PATTERNS) == 12
    for pattern, name in enumerate(fc.PATTERNS):
        users, seen, masks = fc.case_rows(f, bias, cls, pattern)
        assert masks.shape == (N_USERS, N_ITEMS) and masks.dtype == bool
        size = masks.sum(axis=1)
        lo, hi = MASK_SIZE[name]
        assert lo <= size.min() and size.max() <= hi, (name, size.min(), size.max())
        if name == "without the 50 best":
            assert (size == 250).any() and (size == 300).any()     # rows with 50 unseen items to lose, and rows that have seen all
        if name in ("random 30%", "random 1%", "one tile", "all but one tile", "without the 50 best"):
            assert len(np.unique(masks, axis=0)) > 1                # a mask per row
        if name == "word edges":
            assert np.flatnonzero(masks[0]).tolist() == [31, 32, 63, 64]
        eligible = np.array([len(np.setdiff1d(np.flatnonzero(m), s)) for m, s in zip(masks, seen)])
        for topn in TOPNS:
            # a row with nothing left; where the mask can hold that many, a row with topn or more; a row with some but fewer
            assert (eligible == 0).any(), (name, topn)
            if lo >= topn and name != "random 1%":
                assert (eligible >= topn).any(), (name, topn)
            assert (eligible < topn).any(), (name, topn)
            # (losing its 50 best leaves a row of _seen_rows nothing or at least 144 items: that pattern's short rows are empty)
            if topn > 1 and hi > 0 and name != "without the 50 best":
                assert ((eligible > 0) & (eligible < topn)).any(), (name, topn)
        bits, allow_idx = fc.bits_of(pattern, masks)
        assert (allow_idx is None) == (len(np.unique(masks, axis=0)) == 1)
        assert np.array_equal(fc.unpack(bits, N_ITEMS), masks if allow_idx is not None else masks[:1])
        dead = bits[:, -1] >> np.uint32(N_ITEMS % 32)
        assert (dead == (2 ** 20 - 1 if name == "dead bits set" else 0)).all()


@pytest.mark.parametrize("n", (1, 31, 32, 33, 300))
def test_bit_packing_round_trips(n):
    from recmodel_amd.wmf_model import pack_allow_masks
    rng = np.random.default_rng(n)
    masks = rng.random((3, n)) < 0.5
    masks[0], masks[1] = True, False
    masks[2, [0, n - 1]] = True
    words = pack_allow_masks(masks)
    assert words.dtype == np.uint32 and words.shape == (3, (n + 31) // 32)
    assert np.array_equal(words, fc.pack(masks)) and np.array_equal(fc.unpack(words, n), masks)
    for g, j in ((2, 0), (2, n - 1)):
        assert (int(words[g, j >> 5]) >> (j & 31)) & 1
    assert words[1].sum() == 0 and int(words[0, -1]) == (1 << ((n - 1) % 32 + 1)) - 1       # no bit past n
    assert np.array_equal(pack_allow_masks(masks[2]), words[2:])                             # a 1-D mask is one row


def _model():
    from recmodel_amd import WMF
    m = WMF(num_items=5, num_users=6, dim=2, gamma=0.1, weighted=True)
    m.users, m.items = np.zeros((6, 2), dtype=np.float32), np.ones((5, 2), dtype=np.float32)
    return m


def test_model_methods_check_the_filter_before_the_gpu(monkeypatch):
    from recmodel_amd import _lib, wmf_model

    def touched():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    m = _model()
    C = sp.random(4, 5, density=0.5, format="csr", random_state=0)
    ok, two = np.array([1, 0, 1, 1, 0], dtype=bool), np.ones((2, 5), dtype=bool)
    calls = {"recommend": (lambda **kw: m.recommend([0, 1, 2], 3, **kw), 3, 5),
             "recommend_for": (lambda **kw: m.recommend_for(C, 3, **kw), 4, 5),
             "similar_items": (lambda **kw: m.similar_items([0, 1, 2], 3, **kw), 3, 5),
             "similar_users": (lambda **kw: m.similar_users([0, 1], 3, **kw), 2, 6)}
    for name, (call, n_batch, n) in calls.items():
        ok = np.arange(n) % 2 == 0
        two = np.ones((2, n), dtype=bool)
        bad = [dict(allow=np.ones(n + 1, dtype=bool)),                                 # wrong length
               dict(allow=np.ones(n - 1, dtype=bool)),
               dict(allow=np.ones(n)),                                                # wrong dtype: float
               dict(allow=np.array([0.0, 1.0])),
               dict(allow=np.array(["a"])),
               dict(allow=np.array([0, n])),                                          # an id out of range
               dict(allow=np.array([-n - 1])),
               dict(allow=np.ones((2, n + 1), dtype=bool), allow_idx=np.zeros(n_batch, dtype=int)),
               dict(allow=np.ones((2, 2, n), dtype=bool)),
               dict(allow=two),                                                       # 2-D without allow_idx
               dict(allow_idx=np.zeros(n_batch, dtype=int)),                          # allow_idx without allow
               dict(allow=ok, allow_idx=np.zeros(n_batch, dtype=int)),                # ... with a 1-D mask
               dict(allow=np.array([0, 1]), allow_idx=np.zeros(n_batch, dtype=int)),  # ... with a list
               dict(allow=two, allow_idx=np.zeros(n_batch + 1, dtype=int)),           # wrong length
               dict(allow=two, allow_idx=np.zeros(n_batch)),                          # wrong dtype
               dict(allow=two, allow_idx=np.zeros((n_batch, 1), dtype=int)),
               dict(allow=two, allow_idx=np.full(n_batch, 2)),                        # out of range
               dict(allow=two, allow_idx=np.full(n_batch, -2))]
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        good = [dict(allow=ok), dict(allow=ok.tolist()), dict(allow=[0, 3, 3, -1]), dict(allow=np.array([n - 1, 0], dtype=np.uint8)),
                dict(allow=[]), dict(allow=two, allow_idx=np.arange(n_batch) % 3 - 1), dict(allow=two, allow_idx=[0] * n_batch), dict()]
        for kw in good:
            with pytest.raises(AssertionError):
                call(**kw)                                           # well-formed: the next thing it does is ask for the GPU
    with pytest.raises(AssertionError):
        m.recommend([0], wmf_model.RECOMMEND_MAX_TOPN + 1, allow=[0, 1])                # recommend keeps its path beyond the cap
    for call in (m.similar_items, m.similar_users):
        with pytest.raises(ValueError):
            call([0], wmf_model.RECOMMEND_MAX_TOPN + 1, allow=[0, 1])
    with pytest.raises(ValueError):
        m.recommend_for(C, wmf_model.RECOMMEND_MAX_TOPN + 1, allow=[0, 1])


def test_allow_is_canonical():
    from recmodel_amd.wmf_model import _Allow
    a = _Allow([4, -1, 2, 2, 0, -5], None, 5, 3, "item")
    assert a.ids.dtype == np.int32 and a.ids.tolist() == [0, 2, 4] and a.masks is None and not a.empty
    assert _Allow([], None, 5, 3, "item").empty and _Allow(np.zeros(0, dtype=np.int64), None, 5, 3, "item", as_mask=True).empty
    m = _Allow([4, 2], None, 5, 3, "item", as_mask=True)
    assert m.ids is None and m.masks.tolist() == [[False, False, True, False, True]] and m.allowed(1).tolist() == [2, 4]
    g = _Allow(np.eye(2, 5, dtype=bool), [1, -1, 0], 5, 3, "item")
    assert g.idx.dtype == np.int32 and [g.allowed(b).tolist() for b in range(3)] == [[1], [0, 1, 2, 3, 4], [0]]


def test_header_and_ctypes_table_hold_the_new_entry_points():
    from recmodel_amd import _lib
    header = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, after in (("wmf_recommend_topn_filtered", "wmf_recommend_topn"), ("wmf_similar_topn_filtered", "wmf_similar_topn")):
        decl = re.search(rf"int {name}\((.*?)\);", code, flags=re.S).group(1)
        old = re.search(rf"int {after}\((.*?)\);", code, flags=re.S).group(1)
        args, old_args = [a.strip() for a in decl.split(",")], [a.strip() for a in old.split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(args) and restype is _lib.c_int
        for a, t in zip(args, argtypes):
            assert t is (_lib.c_vp if "*" in a else _lib.c_i64 if a.startswith("int64_t") else _lib.c_int), (name, a)
        added = [a for a in args if a not in old_args]
        assert [a.split()[-1].lstrip("*") for a in added][:4] == ["allow_bits", "allow_words", "n_masks", "allow_idx"]
        assert [a for a in args if a in old_args] == old_args           # the old arguments, in their order
        assert hasattr(_lib.load(), name)
    assert int(re.search(r"#define\s+WMF_RECOMMEND_MAX_TOPN\s+(\d+)", header).group(1)) == 128
