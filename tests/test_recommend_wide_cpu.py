"""What wmf_recommend_topn_wide and WMF.candidates / candidates_for promise without a GPU: the two symbols in the header and in the
ctypes table, the argument list of the filtered entry point name for name, the limits, the workspace function against the formula
the header documents, and the argument checks of the Python methods, which all come before the GPU is asked for."""
import os
import re

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def _define(name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", HEADER).group(1))


def _args(name):
    return [a.strip() for a in re.search(rf"int {name}\((.*?)\);", CODE, flags=re.S).group(1).split(",")]


def test_header_and_ctypes_table_hold_the_two_symbols():
    from recmodel_amd import _lib
    wide, filtered = _args("wmf_recommend_topn_wide"), _args("wmf_recommend_topn_filtered")
    assert wide == filtered                                          # the same arguments, name for name, in the same order
    restype, argtypes = _lib.SIGNATURES["wmf_recommend_topn_wide"]
    assert restype is _lib.c_int and list(argtypes) == list(_lib.SIGNATURES["wmf_recommend_topn_filtered"][1]) and len(argtypes) == len(wide)
    for a, t in zip(wide, argtypes):
        assert t is (_lib.c_vp if "*" in a else _lib.c_i64 if a.startswith("int64_t") else _lib.c_int), a
    assert re.search(r"int64_t wmf_recommend_wide_workspace_bytes\(int64_t n_users, int64_t topn, int32_t n_slices\);", CODE)
    assert _lib.SIGNATURES["wmf_recommend_wide_workspace_bytes"] == _lib.SIGNATURES["wmf_recommend_workspace_bytes"]
    lib = _lib.load()
    assert hasattr(lib, "wmf_recommend_topn_wide") and hasattr(lib, "wmf_recommend_wide_workspace_bytes")


def test_limits():
    from recmodel_amd import wmf_model
    assert _define("WMF_RECOMMEND_WIDE_MAX_TOPN") == wmf_model.CANDIDATES_MAX == 4096
    assert _define("WMF_RECOMMEND_MAX_TOPN") == wmf_model.RECOMMEND_MAX_TOPN == 128
    assert wmf_model.CANDIDATES_WS_BYTES == 1 << 30


def _formula(n_users, topn, n_slices):
    """The header's: BASE + L (PER_KEY CAP(topn) + PER_LIST), L = n_users n_slices, or min(AUTO_SLICES n_users, max(AUTO_LISTS,
    n_users)) for n_slices = 0."""
    d = {n: _define("WMF_RECOMMEND_WIDE_" + n) for n in ("WS_BASE", "WS_PER_KEY", "WS_PER_LIST", "AUTO_SLICES", "AUTO_LISTS")}
    assert "#define WMF_RECOMMEND_WIDE_CAP(topn) (2 * (topn) > 32 ? 2 * (topn) : 32)" in HEADER
    cap = max(2 * topn, 32)
    lists = n_users * n_slices if n_slices else min(d["AUTO_SLICES"] * n_users, max(d["AUTO_LISTS"], n_users))
    return d["WS_BASE"] + lists * (d["WS_PER_KEY"] * cap + d["WS_PER_LIST"])


def test_workspace_function():
    from recmodel_amd import _lib
    ws = _lib.load().wmf_recommend_wide_workspace_bytes
    users, topns, slices = (1, 16, 64, 65, 511, 512, 513, 2048, 4096, 32768, 40000), (1, 15, 16, 17, 128, 129, 1000, 4095, 4096), (0, 1, 2, 7, 64, 256)
    for n in users:
        for t in topns:
            for s in slices:
                assert ws(n, t, s) == _formula(n, t, s), (n, t, s)
    # grows with each of its arguments (the forced slice counts among themselves)
    for t in topns:
        for s in slices:
            got = [ws(n, t, s) for n in range(1, 1500)] + [ws(n, t, s) for n in (2048, 4096, 32768, 40000)]
            assert all(a <= b for a, b in zip(got, got[1:])), (t, s)
    for n in users:
        for s in slices:
            got = [ws(n, t, s) for t in range(1, 4097)]
            assert all(a <= b for a, b in zip(got, got[1:])), (n, s)
        for t in topns:
            got = [ws(n, t, s) for s in range(1, 257)]
            assert all(a < b for a, b in zip(got, got[1:])), (n, t)
            assert ws(n, t, 0) <= ws(n, t, 64)                       # the automatic count is at most AUTO_SLICES
    # a buffer holds a tile more than topn, and the catalogue is no argument
    for t in topns:
        assert max(2 * t, 32) >= t + 16
    assert _lib.SIGNATURES["wmf_recommend_wide_workspace_bytes"][1] == [_lib.c_i64, _lib.c_i64, _lib.c_int]


def _model(bias=False, users=True):
    from recmodel_amd import WMF
    m = WMF(num_items=30, num_users=20, dim=4, gamma=0.1, weighted=True, bias=bias)
    if users:
        m.users = np.random.default_rng(0).random((20, m.items.shape[1])).astype(np.float32)
    return m


def _no_gpu(monkeypatch):
    from recmodel_amd import _lib

    def touched():
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", touched)


@pytest.mark.parametrize("bias", (False, True))
def test_argument_checks_come_before_the_gpu(monkeypatch, bias):
    from recmodel_amd import wmf_model
    _no_gpu(monkeypatch)
    m = _model(bias)
    C = scipy.sparse.random(5, 30, 0.2, format="csr", random_state=1, dtype=np.float32)
    for n in (0, -1, wmf_model.CANDIDATES_MAX + 1):
        with pytest.raises(ValueError, match="between 1 and 4096"):
            m.candidates([0, 1], n)
        with pytest.raises(ValueError, match="between 1 and 4096"):
            m.candidates_for(C, n)
    mask2 = np.ones((2, 30), dtype=bool)
    for call, rows in ((lambda **k: m.candidates([0, 1, 2, 3, 4], 200, **k), 5), (lambda **k: m.candidates_for(C, 200, **k), 5)):
        for bad in (dict(allow=np.ones(29, dtype=bool)), dict(allow=[0, 30]), dict(allow=mask2), dict(allow=mask2, allow_idx=[0, 1]),
                    dict(allow=mask2, allow_idx=[0, 1, 2, 0, 0]), dict(allow=np.ones(30, dtype=bool), allow_idx=[0] * rows),
                    dict(allow_idx=[0] * rows), dict(allow=np.ones(30))):
            with pytest.raises(ValueError):
                call(**bad)
    with pytest.raises(ValueError, match="exclude"):
        m.candidates([0], 200, exclude=scipy.sparse.csr_matrix((19, 30)))
    with pytest.raises(IndexError):
        m.candidates([20], 200)
    for bad_rows in (np.zeros((5, 30)), scipy.sparse.csr_matrix((5, 29)), None):
        with pytest.raises(ValueError, match="count_rows"):
            m.candidates_for(bad_rows, 200)
    with pytest.raises(ValueError, match="Pre_process_count"):
        m.candidates_for(C, 200, pre_process_count="sqrt")
    # well-formed calls reach the device: candidates at both ends of its range, recommend just past the LDS kernels' limit
    for call in (lambda: m.candidates([0, -1], 1), lambda: m.candidates(3, wmf_model.CANDIDATES_MAX, allow=[1, 2, 3]),
                 lambda: m.candidates_for(C, 1), lambda: m.candidates_for(C, wmf_model.CANDIDATES_MAX, allow=mask2, allow_idx=[0, 1, -1, 0, 1]),
                 lambda: m.recommend([0], 129), lambda: m.recommend([0], wmf_model.CANDIDATES_MAX + 1)):
        with pytest.raises(AssertionError, match="GPU was touched"):
            call()
    with pytest.raises(ValueError, match="topn"):                    # the neighbours and recommend_for keep their limit
        m.recommend_for(C, 129)
    with pytest.raises(ValueError, match="topn"):
        m.similar_items([0], 129)


def test_an_untrained_model_is_refused_before_the_gpu(monkeypatch):
    _no_gpu(monkeypatch)
    m = _model(users=False)
    assert m.users is None
    C = scipy.sparse.random(5, 30, 0.2, format="csr", random_state=1, dtype=np.float32)
    with pytest.raises((AttributeError, ValueError)):
        m.candidates([0], 200)
    with pytest.raises(ValueError, match="no factors"):
        m.candidates_for(C, 200)


def test_the_docstrings_state_the_limit():
    from recmodel_amd import WMF
    for method in (WMF.candidates, WMF.candidates_for):
        assert "CANDIDATES_MAX" in method.__doc__ and "4096" in method.__doc__ and "ValueError" in method.__doc__
    assert "CANDIDATES_MAX" in WMF.recommend.__doc__ and "4096" in WMF.recommend.__doc__
    assert "WMF_RECOMMEND_WIDE_MAX_TOPN" in HEADER and "1 <= topn <= WMF_RECOMMEND_WIDE_MAX_TOPN" in HEADER
