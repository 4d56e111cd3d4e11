"""What wmf_recommend_topn_grouped and WMF.recommend_shelves / recommend_shelves_for / recommend_capped promise without a GPU: the
references of tests/grouped_ref.py against brute force, every ValueError of the Python methods and every WMF_EINVAL of the entry
point (both before the GPU is asked for), the workspace function against the header's formula, the LDS the scan asks for at the
limit of 64 groups, and the two symbols in the header and in the ctypes table."""
import os
import re

import numpy as np
import pytest
import scipy.sparse

import grouped_ref as gref
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def _define(name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", HEADER).group(1))


# ------------------------------------------------------------------------------------------------------------ the references
def _brute(scores, seen, group_of, g, topn, allow=None):
    seen = set(int(s) for s in seen)
    elig = [j for j in range(len(scores)) if group_of[j] == g and j not in seen and (allow is None or allow[j])]
    return np.array(sorted(elig, key=lambda j: (-scores[j], j))[:topn], dtype=np.int64)


def _rows(seed, n, tied):
    rng = np.random.default_rng(seed)
    scores = rng.integers(-3, 4, n) if tied else rng.standard_normal(n)
    G = int(rng.integers(1, 9))
    group_of = rng.integers(-2, G + 1, n)                            # -2, -1 and G: on no shelf
    seen = rng.choice(n, int(rng.integers(0, n // 2)), replace=False)
    allow = rng.random(n) < 0.7 if seed % 2 else None
    return scores, seen, group_of, G, allow


@pytest.mark.parametrize("tied", (False, True))
def test_grouped_ref_against_a_per_group_sort(tied):
    for seed in range(12):
        scores, seen, group_of, G, allow = _rows(seed, 97, tied)
        for topn in (1, 5, 200):
            got = gref.grouped_ref(scores, seen, group_of, G, topn, allow)
            assert len(got) == G
            for g in range(G):
                assert np.array_equal(got[g], _brute(scores, seen, group_of, g, topn, allow)), (seed, topn, g)


@pytest.mark.parametrize("tied", (False, True))
def test_capped_ref_is_the_merge_of_the_shelves(tied):
    for seed in range(12):
        scores, seen, group_of, G, allow = _rows(100 + seed, 97, tied)
        for topn, per_group in ((10, 1), (10, 2), (10, 10), (10, 50), (1, 3), (97, 4)):
            want = gref.capped_ref(scores, seen, group_of, G, topn, per_group, allow)
            shelves = gref.grouped_ref(scores, seen, group_of, G, min(per_group, topn), allow)
            assert np.array_equal(gref.merge_of_shelves(shelves, scores, topn), want), (seed, topn, per_group)
            assert len(want) <= topn and len(set(want)) == len(want)
            assert all((group_of[want] == g).sum() <= per_group for g in range(G))
            assert not np.isin(want, seen).any() and ((group_of[want] >= 0) & (group_of[want] < G)).all()


def test_capped_ref_with_one_group_and_a_loose_cap_is_the_plain_top_n():
    import recommend_ref as rref
    scores, seen, _, _, _ = _rows(7, 97, True)
    assert np.array_equal(gref.capped_ref(scores, seen, np.zeros(97, dtype=int), 1, 10, 10), rref.recommend_ref(scores, seen, 10))


# ------------------------------------------------------------------------------------------------------ header, table, limits
def test_header_and_ctypes_table_hold_the_two_symbols():
    from recmodel_amd import _lib, wmf_model
    args = [a.strip() for a in re.search(r"int wmf_recommend_topn_grouped\((.*?)\);", CODE, flags=re.S).group(1).split(",")]
    filtered = [a.strip() for a in re.search(r"int wmf_recommend_topn_filtered\((.*?)\);", CODE, flags=re.S).group(1).split(",")]
    at = filtered.index("const int32_t* cand_idx")                   # the filtered call's arguments, group_of / n_groups for the list form's two
    assert args == filtered[:at] + ["const int32_t* group_of", "int32_t n_groups"] + filtered[at + 2:]
    restype, argtypes = _lib.SIGNATURES["wmf_recommend_topn_grouped"]
    assert restype is _lib.c_int and len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        assert t is (_lib.c_vp if "*" in a else _lib.c_i64 if a.startswith("int64_t") else _lib.c_int), a
    assert re.search(r"int64_t wmf_recommend_grouped_workspace_bytes\(int64_t n_users, int32_t n_groups, int64_t topn, int32_t n_slices\);", CODE)
    assert _lib.SIGNATURES["wmf_recommend_grouped_workspace_bytes"] == (_lib.c_i64, [_lib.c_i64, _lib.c_int, _lib.c_i64, _lib.c_int])
    lib = _lib.load()
    assert hasattr(lib, "wmf_recommend_topn_grouped") and hasattr(lib, "wmf_recommend_grouped_workspace_bytes")
    assert _define("WMF_RECOMMEND_GROUPS_MAX") == wmf_model.SHELVES_MAX == 64
    for text in ("bit for bit", "group_of[j] == g", "on no shelf", "only enqueues", "before any HIP call"):
        assert text in HEADER[HEADER.index("One list per (row, GROUP)"):HEADER.index("#define WMF_RECOMMEND_GROUPS_MAX")], text


def _formula(n_users, n_groups, topn, n_slices):
    d = {n: _define("WMF_RECOMMEND_WIDE_" + n) for n in ("WS_BASE", "WS_PER_KEY", "WS_PER_LIST", "AUTO_SLICES", "AUTO_LISTS")}
    assert "#define WMF_RECOMMEND_WIDE_CAP(topn) (2 * (topn) > 32 ? 2 * (topn) : 32)" in HEADER
    lists = n_users * n_slices if n_slices else min(d["AUTO_SLICES"] * n_users, max(d["AUTO_LISTS"], n_users))
    return d["WS_BASE"] + n_groups * lists * (d["WS_PER_KEY"] * max(2 * topn, 32) + d["WS_PER_LIST"])


def test_workspace_function():
    from recmodel_amd import _lib
    lib = _lib.load()
    ws, wide = lib.wmf_recommend_grouped_workspace_bytes, lib.wmf_recommend_wide_workspace_bytes
    users, groups, topns, slices = (1, 16, 64, 65, 512, 513, 2048, 4096, 40000), (1, 2, 3, 31, 32, 33, 64), (1, 10, 16, 17, 127, 128), (0, 1, 2, 7, 64, 256)
    for n in users:
        for t in topns:
            for s in slices:
                assert ws(n, 1, t, s) == wide(n, t, s), (n, t, s)    # one group: the wide call's workspace
                for g in groups:
                    assert ws(n, g, t, s) == _formula(n, g, t, s), (n, g, t, s)
    for s in slices:                                                 # grows with each of its arguments
        for t in topns:
            for g in groups:
                got = [ws(n, g, t, s) for n in list(range(1, 70)) + [500, 511, 512, 513, 600, 2048, 4096, 40000]]
                assert all(a <= b for a, b in zip(got, got[1:])), (g, t, s)
        for n in users:
            for g in groups:
                got = [ws(n, g, t, s) for t in range(1, 129)]
                assert all(a <= b for a, b in zip(got, got[1:])), (n, g, s)
            for t in topns:
                got = [ws(n, g, t, s) for g in range(1, 65)]
                assert all(a < b for a, b in zip(got, got[1:])), (n, t, s)
    for n in users:
        got = [ws(n, 16, 10, s) for s in range(1, 257)]
        assert all(a < b for a, b in zip(got, got[1:])), n


def test_the_scan_fits_its_lds_at_64_groups_in_every_width_class():
    text = open(os.path.join(ROOT, "recmodel_amd", "csrc", "wmf_topn_wide.h")).read()
    waves = int(re.search(r"#define\s+WMF_REC_WIDE_WAVES\s+(\d+)", text).group(1))
    grouped = open(os.path.join(ROOT, "recmodel_amd", "csrc", "wmf_topn_grouped.h")).read()
    assert "(size_t)nw * 16 * n_groups * 12 + (size_t)nw * 256 * 4" in grouped
    launch = open(os.path.join(ROOT, "recmodel_amd", "csrc", "wmf_recommend.hip")).read()
    # the one launch site of the grouped scan: under the 112 KB ceiling, with the LDS of rec_grouped_lds_bytes, and MASK both
    # false and true -- the forms 0 and 1 of the dispatch it sits in
    assert launch.count("recommend_scan_grouped_kernel<NIT, TPS, NW, MASK>), 112 * 1024") == 1
    site = launch[launch.index("int wmf_launch_recommend_grouped("):]
    site = site[:site.index("recommend_scan_grouped_kernel<NIT, TPS, NW, MASK>), 112 * 1024") + 400]
    assert site.count("wmf_dispatch_list<0, 1>(rec_form(flt), [&](auto form) {") == 1
    assert site.count("constexpr bool MASK = decltype(form)::value == 1;") == 1
    assert site.count("wmf_scan_stage_bytes(TPS, ld) + rec_grouped_lds_bytes(NW, n_groups), st,") == 1
    for tps, ld in gref.WIDTH_CLASSES:
        assert gref.scan_lds_bytes(tps, ld, waves, 64) <= 112 * 1024, (tps, ld)
        assert gref.scan_lds_bytes(tps, ld, waves, 64) - gref.scan_lds_bytes(tps, ld, waves, 63) == 768


# ------------------------------------------------------------------------------------------------------------- WMF_EINVAL
def test_every_refusal_of_the_entry_point_without_a_device():
    """The pointers are never followed by a refused call: a made-up address stands for a device array, None for NULL."""
    from recmodel_amd import _lib
    lib = _lib.load()
    P = 4096                                                         # stands for a device pointer
    f, ld, bias, nu, ni, G, topn = 5, 8, 1, 40, 300, 4, 10
    need = lib.wmf_recommend_grouped_workspace_bytes(nu, G, topn, 0)
    ok = dict(users=P, items=P, f=f, ld=ld, bias=bias, user_idx=P, n_users=nu, n_items=ni, seen_indptr=None, seen_indices=None,
              allow_bits=None, allow_words=0, n_masks=0, allow_idx=None, group_of=P, n_groups=G, topn=topn, n_slices=0, out_items=P,
              out_scores=None, out_count=None, workspace=P, workspace_bytes=need, stream=None)

    def call(**over):
        return lib.wmf_recommend_topn_grouped(*{**ok, **over}.values())
    bad = [dict(group_of=None), dict(users=None), dict(items=None), dict(user_idx=None), dict(out_items=None), dict(workspace=None),
           dict(n_groups=0), dict(n_groups=-1), dict(n_groups=65), dict(topn=0), dict(topn=129), dict(n_slices=-1), dict(n_slices=257),
           dict(n_users=0), dict(n_items=0), dict(n_items=2 ** 31), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
           dict(allow_bits=P, allow_words=10, n_masks=0), dict(allow_bits=P, allow_words=9, n_masks=1), dict(allow_idx=P),
           dict(f=0), dict(ld=6), dict(ld=4)]
    for over in bad:
        assert call(**over) == _lib.WMF_EINVAL, over
        assert lib.wmf_last_error(), over
    # (the workspace a refused size would need is never computed from garbage: the refusal of n_groups comes first)
    assert call(n_groups=65, workspace_bytes=0) == _lib.WMF_EINVAL


# ------------------------------------------------------------------------------------------------------ the Python methods
def _model(bias=False):
    from recmodel_amd import WMF
    m = WMF(num_items=30, num_users=20, dim=4, gamma=0.1, weighted=True, bias=bias)
    m.users = np.random.default_rng(0).random((20, m.items.shape[1])).astype(np.float32)
    return m


def _no_gpu(monkeypatch):
    from recmodel_amd import _lib

    def touched():
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)


@pytest.mark.parametrize("bias", (False, True))
def test_argument_checks_come_before_the_gpu(monkeypatch, bias):
    _no_gpu(monkeypatch)
    m = _model(bias)
    C = scipy.sparse.random(5, 30, 0.2, format="csr", random_state=1, dtype=np.float32)
    groups = np.arange(30) % 4
    calls = (lambda g, **k: m.recommend_shelves([0, 1, 2, 3, 4], g, **k), lambda g, **k: m.recommend_shelves_for(C, g, **k))
    for call in calls:
        for g, k in ((groups[:29], {}), (np.append(groups, 0), {}), (groups.astype(np.float32), {}), (groups > 1, {}),
                     (groups.reshape(5, 6), {}), (np.full(30, -1), {}), (groups, dict(n_groups=0)), (groups, dict(n_groups=65)),
                     (groups, dict(n_groups=3)), (np.arange(30) * 3, {}), (groups, dict(topn=0)), (groups, dict(topn=129)),
                     (groups, dict(allow=np.ones(29, dtype=bool))), (groups, dict(allow=[0, 30])), (groups, dict(allow=np.ones((2, 30), dtype=bool))),
                     (groups, dict(allow=np.ones((2, 30), dtype=bool), allow_idx=[0, 1])), (groups, dict(allow_idx=[0] * 5))):
            with pytest.raises(ValueError):
                call(g, **k)
    with pytest.raises(ValueError, match="exclude"):
        m.recommend_shelves([0], groups, exclude=scipy.sparse.csr_matrix((19, 30)))
    with pytest.raises(IndexError):
        m.recommend_shelves([20], groups)
    with pytest.raises(ValueError, match="count_rows"):
        m.recommend_shelves_for(np.zeros((5, 30)), groups)
    for k in (dict(topn=0), dict(topn=129), dict(per_group=0)):
        with pytest.raises(ValueError):
            m.recommend_capped([0], groups, **k)
    with pytest.raises(ValueError):
        m.recommend_capped([0], groups[:29])
    # well-formed calls reach the device
    for call in (lambda: m.recommend_shelves([0, -1], groups), lambda: m.recommend_shelves(3, groups, 128, n_groups=64, allow=[1, 2, 3]),
                 lambda: m.recommend_shelves([0], np.where(groups == 0, -5, groups)), lambda: m.recommend_shelves_for(C, groups, 1),
                 lambda: m.recommend_capped([0, 1], groups, 10, 200), lambda: m.recommend_capped(0, groups, 128, 1)):
        with pytest.raises(AssertionError, match="GPU was touched"):
            call()


def test_the_docstrings_say_what_the_calls_do():
    from recmodel_amd import WMF
    assert "SHELVES_MAX" in WMF.recommend_shelves.__doc__ and "ValueError" in WMF.recommend_shelves.__doc__
    assert "NOT eligible" in WMF.recommend_capped.__doc__
    assert "fold_in(count_rows)" in WMF.recommend_shelves_for.__doc__
