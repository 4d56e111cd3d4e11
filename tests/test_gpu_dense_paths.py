"""The paths inside the split-bf16 dense kernels of the wide factors (csrc/wmf_dense.hip: transform6_kernel, gram6_kernel;
f = 97 .. 144), through the C ABI.

transform6_kernel launches one workgroup per compute unit, each of which splits W into its LDS planes once and then walks
16-row blocks with a grid stride; a block that lies wholly inside the matrix stores without row tests, the one ragged block of
a launch takes the tested path.  gram6_kernel alternates two register sets for a wave's chunks of 32 rows and masks rows only
in the last chunk of a wave.  Neither may show in a result: a row's output depends on neither the row count nor the path that
produced it, nothing is written outside the arrays, and inputs whose answer is a float32 / integer number come out EXACT at
every row -- a stride, grid or staging slip anywhere in the matrix, a swapped register set or a mask in the wrong chunk is a
non-zero difference.

Widths: 97, 112, 113, 128, 129, 144 at the library's ld -- NFB 7, 8 and 9, with one live column in the last block and with a
full one; 97, 113 (not split) and 129 (split, rolled) cover the layouts of the bias column."""
import numpy as np
import pytest
import torch

from test_gpu_dense import (SENT, TAIL, U, _api, _bits, _check_rolled, _dev, _graded, _padded, _rolled_whitening,
                            _signed_permutation, _tilde, _transform)

pytestmark = pytest.mark.gpu

WIDTHS = (97, 112, 113, 128, 129, 144)
FMAX = 144
# 2500 blocks of 16 rows for at most 256 x 8 waves: every wave walks its stride at least once past the first pass and the last
# block is full; seven rows fewer: the last block is ragged; 13 rows: the ragged block is the only one
M1, M2, M3 = 40_000, 40_000 - 7, 13

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ----------------------------------------------------------------------------------------------------------- row transform
def _modes(lib, f, ld):
    """set_col0_one values of wmf_row_transform at this width: plain, the bias mode (whatever layout it resolves to) and the
    rolled pair where the library has it."""
    return [0, 1] + ([3, 4] if lib.wmf_rolled_layout_supported(f, ld) else [])


def _raw_transform(Xd, m, f, ld, Wd, sc):
    """One call on the first m rows of Xd into sentinel-filled outputs.  Returns (rows [m, wid], col0 [nc0] or None) on the
    device after checking that nothing behind them was written."""
    _lib, lib, _ptr, _stream = _api()
    packed = sc == 3 or (sc == 1 and lib.wmf_whitened_row_floats(f, ld, 1) == f - 1)
    wid = f - 1 if packed else ld
    nc0 = 2 * m if packed else m
    out = torch.full((m * wid + 2 * ld,), SENT, device="cuda")
    c0 = torch.full((nc0 + TAIL,), SENT, device="cuda") if sc in (1, 3) else None
    _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), sc, _ptr(out), _ptr(c0), _stream()))
    assert bool((out[m * wid:] == SENT).all()), (f, sc, m, "written behind row m of out")
    if c0 is not None:
        assert bool((c0[nc0:] == SENT).all()), (f, sc, m, "written behind col0_out")
        c0 = c0[:nc0]
    return out[: m * wid].view(m, wid), c0


def _triangular(f, seed, lower, dense=False):
    W = np.random.default_rng(seed).standard_normal((f, f)).astype(np.float32)
    if dense:
        return W
    return np.tril(W) if lower else np.triu(W)


@pytest.mark.parametrize("f", WIDTHS)
def test_transform_row_depends_on_neither_m_nor_path(f):
    """Gaussian input, W upper triangular (lower for the rolled input, mode 4) and once dense, every mode of the width.  m = 40 000
    (all blocks full), 39 993 (ragged last block), 13 (the ragged block alone): the rows and the bias copies that two calls
    share are BITWISE equal, two runs of a call are bitwise equal, and the sentinels behind row m of `out` and behind entry
    m (2 m for the pairs) of col0_out are untouched."""
    _lib, lib, _ptr, _stream = _api()
    ld = lib.wmf_ld_for(f)
    X = _cached("gauss", lambda: np.random.default_rng(40).standard_normal((M1, FMAX), dtype=np.float32))[:, :f]
    Xd = _dev(_padded(X, ld))
    ran = 0
    for sc in _modes(lib, f, ld):
        for dense in (False, True):
            Wd = _dev(_padded(_triangular(f, 5 * f + sc, lower=(sc == 4), dense=dense), ld))
            got = {}
            for m in (M1, M2, M3):
                rows, c0 = _raw_transform(Xd, m, f, ld, Wd, sc)
                rows2, c02 = _raw_transform(Xd, m, f, ld, Wd, sc)
                assert _same_bits(rows, rows2) and (c0 is None or _same_bits(c0, c02)), (f, sc, dense, m, "two runs differ")
                assert (c0 is not None) == (sc in (1, 3))
                got[m] = (rows, c0)
            per_row = 0 if got[M1][1] is None else got[M1][1].numel() // M1
            for m in (M2, M3):
                assert _same_bits(got[M1][0][:m], got[m][0]), (f, sc, dense, m, "rows depend on m")
                assert _same_bits(got[M2][0][:M3], got[M3][0]), (f, sc, dense, m)
                if per_row:
                    assert _same_bits(got[M1][1][: per_row * m], got[m][1]), (f, sc, dense, m, "col0_out depends on m")
            assert bool(got[M1][0].abs().sum() > 0)
            ran += 1
    assert ran == 2 * (2 + 2 * (f == 129))


@pytest.mark.parametrize("f", WIDTHS)
def test_transform_is_exact_at_every_row_of_a_long_matrix(f):
    """W a signed power-of-two permutation (rolled accordingly by the rolled modes), Gaussian input, m = 40 000: the output
    EQUALS the NumPy permutation at every row of every mode -- the three bf16 parts of a float32 recombine exactly, so a
    block that no wave took, one that two took, or a slip in any staged plane of W is a non-zero difference."""
    _lib, lib, _ptr, _stream = _api()
    ld = lib.wmf_ld_for(f)
    X = _graded(M1, f, seed=23 * f)
    for sc in _modes(lib, f, ld):
        W, pi, val = _signed_permutation(f, seed=7 * f + sc, fix0=(sc == 3))
        ref = np.zeros((M1, f), dtype=np.float32)
        ref[:, pi] = _tilde(X, sc in (1, 3), np.float32) * val[None, :]
        if sc == 3:
            got3, body3, pairs3 = _rolled_whitening(X, W, ld)
            plain, _ = _transform(X, W, "1", ld)
            assert np.array_equal(plain, ref)
            _check_rolled(got3, body3, pairs3, plain, X)
            continue
        got, c0 = _transform(X, W, str(sc), ld)
        bad = np.argwhere(got != ref)
        assert not len(bad), (f, sc, len(bad), bad[:4].tolist(), [(got[i, j], ref[i, j]) for i, j in bad[:4]])
        if sc == 1:
            assert np.array_equal(_bits(c0), _bits(X[:, 0]))


# ------------------------------------------------------------------------------------------------------------------ Gramian
GRAM_SMALL = (1, 31, 32, 33, 64, 65, 96, 97, 160, 161)     # one wave, 1 .. 6 chunks: both register sets, last chunk full and ragged
GRAM_BIG = (140_000, 200_003)                              # 1024 waves of 4 - 5 and 6 - 7 chunks: both parities in one launch
MBIG = max(GRAM_BIG)


def _int_base():
    return _cached("int", lambda: np.random.default_rng(41).integers(-3, 4, (MBIG, FMAX)).astype(np.float32))


def _gauss_base():
    return _cached("gaussbig", lambda: np.random.default_rng(42).standard_normal((MBIG, FMAX), dtype=np.float32))


def _reference(kind, m, f, bias):
    """float64 Gramian of the first m rows and f columns of a base, column 0 read as one for a bias model, and the same of the
    absolute values: one [144, 144] product per (base, m), shared by every width (a leading block of it) and both bias
    settings (only row and column 0 change: the column sums and m)."""
    def make():
        Y = (_int_base() if kind == "int" else _gauss_base())[:m].astype(np.float64)
        return Y.T @ Y, Y.sum(axis=0), np.abs(Y).T @ np.abs(Y), np.abs(Y).sum(axis=0)
    G, s, A, a = _cached(("ref", kind, m), make)
    G, A = G[:f, :f].copy(), A[:f, :f].copy()
    if bias:
        G[0, :] = G[:, 0] = s[:f]
        A[0, :] = A[:, 0] = a[:f]
        G[0, 0] = A[0, 0] = m
    return G, A


def _gram_device(kind, m, f, bias):
    """wmf_gram twice on the first m rows of a base (kept on the device); with a bias, column 0 holds 1e30 -- it reads as one
    and must not be read as data."""
    _lib, lib, _ptr, _stream = _api()
    ld = lib.wmf_ld_for(f)
    base = _cached(("dev", kind), lambda: _dev(_int_base() if kind == "int" else _gauss_base()))
    Yd = torch.zeros(m, ld, device="cuda")
    Yd[:, :f] = base[:m, :f]
    if bias:
        Yd[:, 0] = 1e30
    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    out = []
    for _ in range(2):
        G = torch.full((f * f,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.wmf_gram(_ptr(Yd), m, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
        out.append(G.cpu().numpy().reshape(f, f))
    assert np.array_equal(out[0], out[1]), (kind, m, f, bias, "two runs differ")
    return out[0]


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", WIDTHS)
def test_gramian_is_exact_on_integers_at_every_chunk_count(f, bias):
    """Integer factors in -3 .. 3: every product and every partial sum is an integer below 2^24 (and the float64 reference an
    integer below 2^53: it is exact, and compared as int64), so G must EQUAL it -- at one wave with 1 .. 6 chunks (both
    register sets, the wave's last chunk full and ragged) and at 1024 waves with 4 - 5 and 6 - 7 chunks each (both parities in
    one launch, the ragged chunk of the matrix in either register set)."""
    for m in GRAM_SMALL + GRAM_BIG:
        G = _gram_device("int", m, f, bias)
        Gref, _ = _reference("int", m, f, bias)
        assert np.array_equal(Gref, np.rint(Gref)) and np.abs(Gref).max() < 2.0 ** 24
        bad = np.argwhere(G.astype(np.int64) != Gref.astype(np.int64))
        assert np.array_equal(G, np.rint(G)) and not len(bad), (f, bias, m, len(bad), bad[:4].tolist(),
                                                                  [(G[i, j], Gref[i, j]) for i, j in bad[:4]])


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", WIDTHS)
def test_gramian_of_gaussian_factors_at_200003_rows(f, bias):
    """Gaussian factors, m = 200 003, against the float64 product: per element |G - Gref| <= 2 (m + 2) u (|Y|^T |Y|), the
    few-term bound of tests/test_gpu_dense.py for the split-bf16 Gramian (m u for an m-term float32 dot product in any order,
    one u each for the dropped products of the split and the final rounding, doubled for a truncating accumulator) at this m."""
    m = MBIG
    G = _gram_device("gauss", m, f, bias)
    Gref, mag = _reference("gauss", m, f, bias)
    assert np.all(mag > 0)
    ratio = np.abs(G - Gref) / (mag * U)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"gram gaussian f={f} bias={bias} m={m}: worst {ratio.max():.3f} u of a bound of {2 * (m + 2)} u")
    assert ratio.max() <= 2 * (m + 2), (f, bias, (int(i), int(j)), float(ratio.max()), G[i, j], Gref[i, j])
    assert np.array_equal(G, G.T)
