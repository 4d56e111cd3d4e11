"""What the sampled top-n promises without a GPU: the NumPy reference (tests/sample_ref.py) against a brute-force loop, the ranges of
u and g, the chi-square test of the hash on a small catalogue, the argument checks of WMF.sample_items / sample_items_for /
log_partition -- all before the GPU is asked for -- every WMF_EINVAL of the four entry points, the workspace formulas and the ABI
table."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse
import scipy.stats

import sample_ref as sref
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "wmf_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NOISE_H = open(os.path.join(ROOT, "recmodel_amd", "csrc", "wmf_noise.h")).read()

CHI_SCORES = np.arange(8) * 0.5                                     # the catalogue of the chi-square tests: 0, 0.5, ..., 3.5
CHI_STREAMS, CHI_SEED, CHI_TEMPERATURES = 8192, 1993, (0.5, 1.0, 4.0)


def chi_square_gate(lists, temperature):
    """The issue's gate on [streams, 2] lists over CHI_SCORES: the statistic of the first picks, and of the ordered pairs over the
    cells with expectation >= 5, below the 1 - 10^-6 quantile for cells - 1 degrees of freedom.  Returns the two statistics."""
    lists = np.asarray(lists)
    n, m = len(lists), len(CHI_SCORES)
    assert lists.shape == (n, 2) and (lists[:, 0] != lists[:, 1]).all() and lists.min() >= 0 and lists.max() < m
    first, cells1 = sref.chi_square(np.bincount(lists[:, 0], minlength=m), n * sref.plackett_luce_first(CHI_SCORES, temperature), floor=0.0)
    pairs = np.zeros((m, m))
    np.add.at(pairs, (lists[:, 0], lists[:, 1]), 1)
    second, cells2 = sref.chi_square(pairs, n * sref.plackett_luce_pairs(CHI_SCORES, temperature))
    assert cells1 == m and cells2 >= 20
    assert first < scipy.stats.chi2.ppf(1 - 1e-6, cells1 - 1), (temperature, first)
    assert second < scipy.stats.chi2.ppf(1 - 1e-6, cells2 - 1), (temperature, second, cells2)
    return first, second, cells2


# ----------------------------------------------------------------------------------------------------------- the reference
def _mix_int(z):
    z &= 2 ** 64 - 1
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & (2 ** 64 - 1)
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & (2 ** 64 - 1)
    return z ^ (z >> 31)


def _k_int(seed, stream, item):
    a = _mix_int(seed + 0x9E3779B97F4A7C15 * (stream + 1))
    return _mix_int(a + 0x9E3779B97F4A7C15 * ((item & 0xFFFFFFFF) + 1)) >> 41


def test_the_hash_against_python_integers():
    rng = np.random.default_rng(1)
    edge = [0, 1, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1]
    seeds = edge + [int(x) for x in rng.integers(0, 2 ** 64, 40, dtype=np.uint64)]
    streams = edge + [int(x) for x in rng.integers(0, 2 ** 64, 40, dtype=np.uint64)]
    items = [0, 1, 2 ** 31 - 1, -1, 12345] + [int(x) for x in rng.integers(0, 2 ** 31, 20)]
    for seed in seeds[:12]:
        got = sref.noise_k(seed, np.array(streams, dtype=np.uint64)[:, None], np.array(items)[None, :])
        want = [[_k_int(seed, s, j) for j in items] for s in streams]
        assert got.dtype == np.uint32 and np.array_equal(got, want), seed
    assert sref.noise_k(0, 0, 0) != sref.noise_k(0, 1, 0) != sref.noise_k(1, 0, 0)


def test_the_sampled_list_against_a_brute_force_loop():
    rng = np.random.default_rng(2)
    for trial in range(20):
        n_items, B, n = int(rng.integers(1, 60)), 5, int(rng.integers(1, 12))
        T = float(rng.choice([0.0, 0.25, 1.0, 4.0]))
        scores = rng.integers(-3, 4, (B, n_items)).astype(np.float64)       # many ties
        noise = sref.noise_matrix(trial, np.arange(B), n_items)
        if trial % 3 == 0:
            noise[:] = np.round(noise)                                      # ties in z as well
        seen = [np.flatnonzero(rng.random(n_items) < 0.3) for _ in range(B)]
        got = sref.sample_lists(scores, noise, T, seen, n)
        for b in range(B):
            z = scores[b] + T * noise[b]
            elig = [j for j in range(n_items) if j not in set(seen[b].tolist())]
            want = sorted(elig, key=lambda j: (-z[j], j))[:n]
            assert got[b].tolist() == want, (trial, b)
    # -0.0 equals +0.0: the lower id wins
    assert sref.sample_row(np.array([-0.0, 0.0, -1.0]), [], 2).tolist() == [0, 1]
    assert sref.sample_row(np.array([0.0, -0.0, -1.0]), [], 2).tolist() == [0, 1]


def test_ranges_of_u_and_g():
    k = np.concatenate([[0, 1, sref.K_MAX - 1, sref.K_MAX], np.random.default_rng(3).integers(0, 2 ** 23, 100000)])
    u = sref.noise_u(k)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)       # exact in float32
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    g = sref.noise_g(k)
    assert sref.G_MIN <= g.min() and g.max() <= sref.G_MAX
    assert abs(sref.noise_g(0) - -2.8115409) < 1e-6 and abs(sref.noise_g(sref.K_MAX) - 16.6355323) < 1e-6
    # WMF_SAMPLE_G_MAX is the float32 of g at the last k
    text = re.search(r"#define\s+WMF_SAMPLE_G_MAX\s+(\S+?)f\b", HEADER).group(1)
    assert float.fromhex(text) == float(np.float32(sref.noise_g(sref.K_MAX)))
    kk = sref.noise_k(7, np.arange(64, dtype=np.uint64)[:, None], np.arange(4096)[None, :])
    assert kk.max() <= sref.K_MAX and kk.min() >= 0 and len(np.unique(kk)) > 0.98 * kk.size


def test_the_perturbed_key_is_rounded_once():
    from fractions import Fraction
    rng = np.random.default_rng(4)
    g32 = sref.noise_g(rng.integers(0, 2 ** 23, 400)).astype(np.float32)
    s = rng.integers(-2340, 2341, 400)
    for T in (0.25, 1.0, 4.0):
        z = sref.perturbed_exact(s, T, g32)
        for zi, si, gi in zip(z, s, g32):
            exact = Fraction(int(si)) + Fraction(T) * Fraction(float(gi))
            lo, hi = np.nextafter(zi, np.float32(-np.inf)), np.nextafter(zi, np.float32(np.inf))
            assert abs(Fraction(float(zi)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


@pytest.mark.parametrize("temperature", CHI_TEMPERATURES)
def test_chi_square_of_the_hash(temperature):
    """8192 streams, n = 2, seed 1993 on the reference's float64 noise: Plackett-Luce over eight items."""
    noise = sref.noise_matrix(CHI_SEED, np.arange(CHI_STREAMS), len(CHI_SCORES))
    lists = sref.sample_lists(np.tile(CHI_SCORES, (CHI_STREAMS, 1)), noise, temperature, None, 2)
    first, second, cells = chi_square_gate(lists, temperature)
    print(f"T = {temperature}: first picks {first:.1f} at 7 degrees of freedom, pairs {second:.1f} over {cells} cells")


def test_logsumexp64():
    assert sref.logsumexp64([]) == -np.inf and sref.logsumexp64([-np.inf]) == -np.inf
    assert sref.logsumexp64([0.0, 0.0]) == pytest.approx(math.log(2))
    assert sref.logsumexp64([1000.0, 1000.0, -1000.0]) == pytest.approx(1000 + math.log(2))


# ------------------------------------------------------------------------------------------------- the header and the table
def _args(name):
    return [a.strip() for a in re.search(rf"int {name}\((.*?)\);", CODE, flags=re.S).group(1).split(",")]


def _ctype_of(arg):
    from recmodel_amd import _lib
    if "*" in arg:
        return _lib.c_vp
    return {"int64_t": _lib.c_i64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}.get(arg.split()[0], _lib.c_int)


def test_header_and_ctypes_table():
    from recmodel_amd import _lib
    wide, sample, logz = _args("wmf_recommend_topn_wide"), _args("wmf_sample_topn"), _args("wmf_log_partition")
    rename = lambda a: a.replace("n_users", "n_rows").replace("topn", "n")   # noqa: E731
    assert sample[:18] == [rename(a) for a in wide[:18]]                     # the same arguments up to the slices
    assert sample[18:21] == ["float temperature", "uint64_t seed", "const uint64_t* row_stream"]
    assert sample[21:] == ["int32_t* out_items", "float* out_scores", "float* out_keys", "int32_t* out_count", "void* workspace",
                           "int64_t workspace_bytes", "void* stream"]
    assert logz[:16] == sample[:16] and logz[16:] == ["float temperature", "int32_t n_slices", "float* out_logz", "int32_t* out_eligible",
                                                       "void* workspace", "int64_t workspace_bytes", "void* stream"]
    for name in ("wmf_sample_topn", "wmf_log_partition", "wmf_sample_noise"):
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.c_int and [_ctype_of(a) for a in _args(name)] == list(argtypes), name
    assert _lib.SIGNATURES["wmf_sample_workspace_bytes"] == _lib.SIGNATURES["wmf_recommend_wide_workspace_bytes"]
    assert _lib.SIGNATURES["wmf_log_partition_workspace_bytes"] == (_lib.c_i64, [_lib.c_i64, _lib.c_int])
    lib = _lib.load()
    for name in ("wmf_sample_topn", "wmf_sample_noise", "wmf_sample_workspace_bytes", "wmf_log_partition", "wmf_log_partition_workspace_bytes"):
        assert hasattr(lib, name)


def test_the_header_documents_the_hash_the_order_and_the_tail():
    for text in (HEADER, NOISE_H):
        for piece in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15", "z >> 30", "z >> 27", "z >> 31", "h >> 41",
                      "(stream + 1)", "2^-24", "-logf(-logf(u))", "-2.8116, 16.6356"):
            assert piece in text, piece
    for piece in ("fmaf(temperature, g, score)", "equal z goes to the lower id", "temperature == 0", "bit for bit", "WMF_SAMPLE_G_MAX",
                  "e^-16", "row_stream == NULL"):
        assert piece in HEADER, piece


def test_workspace_functions():
    from recmodel_amd import _lib
    lib = _lib.load()
    base = int(re.search(r"#define\s+WMF_RECOMMEND_WIDE_WS_BASE\s+(\d+)", HEADER).group(1))
    per_lane = int(re.search(r"#define\s+WMF_LOG_PARTITION_WS_PER_LANE\s+(\d+)", HEADER).group(1))
    auto_s, auto_l = (int(re.search(rf"#define\s+WMF_RECOMMEND_WIDE_{n}\s+(\d+)", HEADER).group(1)) for n in ("AUTO_SLICES", "AUTO_LISTS"))
    for rows in (1, 16, 64, 511, 512, 513, 2048, 40000):
        for s in (0, 1, 2, 7, 64, 256):
            lists = rows * s if s else min(auto_s * rows, max(auto_l, rows))
            assert lib.wmf_log_partition_workspace_bytes(rows, s) == base + lists * 16 * per_lane, (rows, s)
            for n in (1, 10, 129, 1000, 4096):
                assert lib.wmf_sample_workspace_bytes(rows, n, s) == lib.wmf_recommend_wide_workspace_bytes(rows, n, s)
    assert lib.wmf_log_partition_workspace_bytes(0, 0) == base == lib.wmf_log_partition_workspace_bytes(4, -1)


# ----------------------------------------------------------------------------------------------- WMF_EINVAL without a device
def test_every_refusal_of_the_entry_points_comes_before_the_device():
    """Never-dereferenced addresses stand for the device pointers: a refusal that came after a HIP call would fault or answer
    WMF_EHIP on a machine without a device."""
    from recmodel_amd import _lib
    lib = _lib.load()
    E, P = _lib.WMF_EINVAL, ctypes.c_void_p(4096)
    f, ld, rows, n_items = 5, 8, 3, 300
    big = 1 << 40

    def sample(**o):
        g = dict(users=P, items=P, f=f, ld=ld, user_idx=P, rows=rows, n_items=n_items, bits=None, words=0, n_masks=0, allow_idx=None, cand=None,
                 n_cand=0, n=10, n_slices=0, T=1.0, out_items=P, ws=P, ws_bytes=big)
        g.update(o)
        return lib.wmf_sample_topn(g["users"], g["items"], g["f"], g["ld"], 1, g["user_idx"], g["rows"], g["n_items"], None, None, g["bits"],
                                   g["words"], g["n_masks"], g["allow_idx"], g["cand"], g["n_cand"], g["n"], g["n_slices"], g["T"], 5, None,
                                   g["out_items"], None, None, None, g["ws"], g["ws_bytes"], None)

    def logz(**o):
        g = dict(users=P, items=P, f=f, ld=ld, user_idx=P, rows=rows, n_items=n_items, bits=None, words=0, n_masks=0, allow_idx=None, cand=None,
                 n_cand=0, n_slices=0, T=1.0, out=P, ws=P, ws_bytes=big)
        g.update(o)
        return lib.wmf_log_partition(g["users"], g["items"], g["f"], g["ld"], 1, g["user_idx"], g["rows"], g["n_items"], None, None, g["bits"],
                                     g["words"], g["n_masks"], g["allow_idx"], g["cand"], g["n_cand"], g["T"], g["n_slices"], g["out"], None,
                                     g["ws"], g["ws_bytes"], None)

    shared = [dict(f=0), dict(f=261), dict(ld=7), dict(ld=4), dict(ld=276), dict(users=None), dict(items=None), dict(user_idx=None), dict(ws=None),
              dict(rows=0), dict(n_items=0), dict(n_items=2 ** 31), dict(n_slices=-1), dict(n_slices=257), dict(bits=P, cand=P, words=10, n_masks=1, n_cand=5),
              dict(bits=P, words=10, n_masks=0), dict(bits=P, words=9, n_masks=1), dict(allow_idx=P), dict(cand=P, n_cand=0),
              dict(cand=P, n_cand=n_items + 1), dict(T=float("nan")), dict(T=float("inf")), dict(T=-1.0), dict(T=-0.5)]
    for bad in shared:
        assert sample(**bad) == E, bad
        assert lib.wmf_last_error()
        assert logz(**bad) == E, bad
    for bad in (dict(n=0), dict(n=4097), dict(out_items=None), dict(ws_bytes=lib.wmf_sample_workspace_bytes(rows, 10, 0) - 1),
                dict(n_slices=3, ws_bytes=lib.wmf_sample_workspace_bytes(rows, 10, 3) - 1)):
        assert sample(**bad) == E, bad
    for bad in (dict(T=0.0), dict(out=None), dict(ws_bytes=lib.wmf_log_partition_workspace_bytes(rows, 0) - 1),
                dict(n_slices=3, ws_bytes=lib.wmf_log_partition_workspace_bytes(rows, 3) - 1)):
        assert logz(**bad) == E, bad
    assert lib.wmf_sample_noise(1, None, None, 4, P, P, None) == E
    assert lib.wmf_sample_noise(1, None, P, -1, P, P, None) == E
    assert lib.wmf_sample_noise(1, None, P, 4, None, None, None) == E
    assert lib.wmf_sample_noise(1, None, P, 0, P, None, None) == _lib.WMF_OK         # nothing to do: no launch either


# -------------------------------------------------------------------------------------------------- the Python methods
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
    calls = ((lambda **k: m.sample_items([0, 1, 2, 3, 4], **k)), (lambda **k: m.sample_items_for(C, **k)))
    for call in calls:
        for n in (0, -1, wmf_model.CANDIDATES_MAX + 1):
            with pytest.raises(ValueError, match="between 1 and 4096"):
                call(n=n)
        for T in (-1.0, float("nan"), float("inf"), -1e-30, 1e39):
            with pytest.raises(ValueError, match="temperature"):
                call(temperature=T)
        with pytest.raises(ValueError, match="temperature"):
            call(temperature=0, return_log_prob=True)
        for seed in (-1, 2 ** 64, 1.5, True):
            with pytest.raises(ValueError, match="seed"):
                call(seed=seed)
        for streams in ([0, 1, 2, 3], [0, 1, 2, 3, 4, 5], [[0, 1, 2, 3, 4]], [0.0, 1, 2, 3, 4], [0, -1, 2, 3, 4], [True] * 5):
            with pytest.raises(ValueError, match="streams"):
                call(streams=streams)
        mask2 = np.ones((2, 30), dtype=bool)
        for bad in (dict(allow=np.ones(29, dtype=bool)), dict(allow=[0, 30]), dict(allow=mask2), dict(allow=mask2, allow_idx=[0, 1]),
                    dict(allow_idx=[0] * 5), dict(allow=np.ones(30))):
            with pytest.raises(ValueError):
                call(**bad)
        for good in (dict(), dict(n=1, temperature=0), dict(n=wmf_model.CANDIDATES_MAX, seed=2 ** 64 - 1), dict(streams=np.arange(5, dtype=np.uint64)),
                     dict(streams=[2 ** 64 - 1, 0, 1, 2, 3], return_log_prob=True), dict(allow=mask2, allow_idx=[0, 1, -1, 0, 1], return_scores=True)):
            with pytest.raises(AssertionError, match="GPU was touched"):
                call(**good)
    with pytest.raises(ValueError, match="exclude"):
        m.sample_items([0], exclude=scipy.sparse.csr_matrix((19, 30)))
    with pytest.raises(IndexError):
        m.sample_items([20])
    for bad_rows in (np.zeros((5, 30)), scipy.sparse.csr_matrix((5, 29)), None):
        with pytest.raises(ValueError, match="count_rows"):
            m.sample_items_for(bad_rows)
    with pytest.raises(ValueError, match="Pre_process_count"):
        m.sample_items_for(C, pre_process_count="sqrt")
    # log_partition
    for T in (0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="temperature"):
            m.log_partition([0, 1], temperature=T)
    with pytest.raises(ValueError, match="exclude"):
        m.log_partition([0], exclude=scipy.sparse.csr_matrix((19, 30)))
    with pytest.raises(IndexError):
        m.log_partition([-21])
    with pytest.raises(ValueError):
        m.log_partition([0, 1], allow=np.ones(29, dtype=bool))
    for call in (lambda: m.log_partition([0, 1]), lambda: m.log_partition(3, temperature=0.1, allow=[1, 2])):
        with pytest.raises(AssertionError, match="GPU was touched"):
            call()


def test_the_docstrings_state_the_contract():
    from recmodel_amd import WMF
    doc = WMF.sample_items.__doc__
    for piece in ("CANDIDATES_MAX", "ValueError", "USER ID", "without replacement", "e^-16", "log Z"):
        assert piece in doc, piece
    assert "position" in WMF.sample_items_for.__doc__ and "fold_in" in WMF.sample_items_for.__doc__
