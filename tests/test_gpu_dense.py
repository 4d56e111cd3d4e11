"""The three dense passes of a half step (csrc/wmf_dense.hip) one by one through the C ABI, per element, at every block count.

wmf_gram, wmf_factorize and wmf_row_transform are templated on NFB = ceil(f / 16) = 1 .. 17 with different kernels per range
(f32 / split-bf16 / four-wave Gramian; W in LDS, split-bf16, two and three column slices, W in global memory for an in-place
call; single-wave and workgroup factorisation).  Everything the row kernels solve is built on their output.  The gates here
are either EXACT -- inputs whose correct answer is a float32 number, so any indexing, masking, slicing, layout or
split-recombination slip is a non-zero difference -- or the textbook bound of a few-term float32 dot product, per element,
which separates 24-bit arithmetic from a product lost in a bf16 split (>= 100 u against a gate of 6 .. 20 u), or RELATIVE TO
NUMPY'S float32 PRODUCT of the same operands, measured in the same test.  References are NumPy float64 (Yt.T @ Yt,
np.linalg.cholesky, Yt @ W) with column 0 read as one for bias models (RecModel/wmf_model.py:215, 328-332).

Widths: for every NFB the width with ONE live column in the last block (16 NFB - 15), an interior one and the full one
(16 NFB), and 257 .. 260 for the three-slice launch; these include every split-layout width (17, 33, 65, 81, 97, 129)."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import record_error
from recmodel_amd._lib import DEBUG_FLAGS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                    # unit roundoff of float32
WMF_MAX_F = 260
M_EDGES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1234)
WIDTHS = sorted({f for n in range(1, 18) for f in (16 * n - 15, 16 * n - 6, 16 * n) if f <= WMF_MAX_F} | {258, 259, 260})
SPLIT_WIDTHS = (17, 33, 65, 81, 97, 129)
assert set(SPLIT_WIDTHS) <= set(WIDTHS) and {(f + 15) // 16 for f in WIDTHS} == set(range(1, 18))
F32_GRAM = DEBUG_FLAGS["WMF_DBG_F32_GRAM"]                        # wmf_debug_set_flags: the f32-MFMA Gramian for NFB 7 .. 9


def _big_m(f):
    """A row count beyond 131 072 (more than 1024 waves wanted: wmf_gram_nwaves rounds, or caps, the count), for one width per
    block count up to the last one whose cap lies above 1024 (NFB 10) and for the two- and three-slice extremes."""
    if f == 64:
        return 140_000
    if f % 16 == 1 and (f <= 145 or f in (193, 257)):
        return 200_003
    return None


def _gram_cases():
    cases = []
    for f in WIDTHS:
        for bias in (0, 1):
            cases.append((f, bias, 0))
            if 7 <= (f + 15) // 16 <= 9:
                cases.append((f, bias, F32_GRAM))
    return cases


GRAM_CASES = _gram_cases()


# ------------------------------------------------------------------------------------------------------------------ helpers
def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@contextlib.contextmanager
def _flags(lib, flags):
    """Kernel-selection switch for the duration of a test; a library that does not offer it (a return of -1) skips the item."""
    if flags and lib.wmf_debug_set_flags(flags) != 0:
        lib.wmf_debug_set_flags(0)
        pytest.skip(f"wmf_debug_set_flags({flags}) is not compiled into this library")
    try:
        yield
    finally:
        lib.wmf_debug_set_flags(0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(Y, ld, extra_rows=0, fill=0.0):
    """[m + extra_rows, ld] float32: Y in the leading columns, zero padding columns, `fill` in the extra rows."""
    m, f = Y.shape
    P = np.zeros((m + extra_rows, ld), dtype=np.float32)
    P[:m, :f] = Y
    P[m:] = fill
    return P


def _tilde(Y, bias, dtype=np.float64):
    Yt = Y.astype(dtype)
    if bias:
        Yt[:, 0] = 1
    return Yt


_CACHE = {}


def _column_scales(f, seed):
    """Per-column scales 2^-10 .. 2^2, every exponent present once f >= 13, in random column order."""
    rng = np.random.default_rng(1000 + seed)
    return (2.0 ** rng.permutation(np.resize(np.arange(-10, 3), f))).astype(np.float32)


def _graded(m, f, seed):
    """Gaussian x per-column scale: the graded column norms of trained factors (column 0 doubles as the bias values)."""
    if m > 5000:                                                  # the large matrices are drawn once and sliced
        key = ("graded", m)
        if key not in _CACHE:
            _CACHE[key] = np.random.default_rng(m).standard_normal((m, WMF_MAX_F), dtype=np.float32)
        base = _CACHE[key][:, :f]
    else:
        base = np.random.default_rng(seed).standard_normal((m, f), dtype=np.float32)
    return base * _column_scales(f, seed)[None, :]


def _integers(m, f, seed):
    """Integers in [-7, 7] with zero rows and a zero column: every product and partial sum is an integer below 2^24."""
    rng = np.random.default_rng(seed)
    if m > 5000:
        key = ("int", m)
        if key not in _CACHE:
            _CACHE[key] = np.random.default_rng(m + 1).integers(-7, 8, (m, WMF_MAX_F), dtype=np.int8)
        Y = _CACHE[key][:, :f].astype(np.float32)
    else:
        Y = rng.integers(-7, 8, (m, f)).astype(np.float32)
    Y[rng.random(m) < 0.1] = 0
    if m >= 3:
        Y[m // 2] = 0
    if f >= 3:
        Y[:, int(rng.integers(1, f))] = 0
    return Y


def _gram(Y, bias, ld=None, calls=1):
    """wmf_gram on Y [m, f] (host); returns the [f, f] float64 result of every call."""
    _lib, lib, _ptr, _stream = _api()
    m, f = Y.shape
    ld = ld or lib.wmf_ld_for(f)
    Yd = _dev(_padded(Y, ld)) if m else torch.zeros(4, ld, device="cuda")
    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    out = []
    for _ in range(calls):
        G = torch.full((f * f,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.wmf_gram(_ptr(Yd), m, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
        out.append(G.cpu().numpy().reshape(f, f))
    return out


def _factorize(G, lam, ld=None, info=None, fill=7.0):
    """wmf_factorize on G [f, f] float64 (host); returns W_white, W_unwhite [f, ld] and the info tensor."""
    _lib, lib, _ptr, _stream = _api()
    f = G.shape[0]
    ld = ld or lib.wmf_ld_for(f)
    Gd = _dev(G.astype(np.float64).reshape(-1))
    Ww, Wu = torch.full((f, ld), fill, device="cuda"), torch.full((f, ld), fill, device="cuda")
    if info is None:
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.wmf_factorize(_ptr(Gd), f, ld, float(lam), _ptr(Ww), _ptr(Wu), _ptr(info), _ptr(ws), _stream()))
    return Ww.cpu().numpy(), Wu.cpu().numpy(), info


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


SENT = 3.0                                                        # sentinel of over-allocated outputs
TAIL = 8


def _modes_of(lib, f, ld):
    """The calls of wmf_row_transform this width supports, from the ABI's own predicates."""
    modes = ["0", "0-in-place", "1"]
    if lib.wmf_whitened_row_floats(f, ld, 1) == f - 1:
        modes.append("1-refusals")                                # split layout: the pairs are required, no aliasing
    else:
        modes.append("1-null")                                    # col0_out = NULL accepted
    if lib.wmf_rolled_layout_supported(f, ld):
        modes += ["3", "4"]
    return modes


def _transform(X, W, mode, ld=None):
    """One wmf_row_transform call in `mode` on X [m, f], W [f, f] (host float32).  Returns the result as a logical [m, f] matrix
    (features in their natural order, whatever layout the call wrote) and the bias copy (or None), after checking the layout's
    own promises: zero padding columns, nothing written behind the arrays, col0_out bitwise."""
    _lib, lib, _ptr, _stream = _api()
    m, f = X.shape
    ld = ld or lib.wmf_ld_for(f)
    Wd = _dev(_padded(W, ld))
    split = lib.wmf_whitened_row_floats(f, ld, 1) == f - 1
    if mode == "4":                                               # the input in rolled coordinates: feature c at position c - 1
        X = np.concatenate([X[:, 1:], X[:, :1]], axis=1)
    if mode == "0-in-place":
        buf = _dev(_padded(X, ld, extra_rows=2, fill=SENT))
        _lib.check(lib.wmf_row_transform(_ptr(buf), m, f, ld, _ptr(Wd), 0, _ptr(buf), None, _stream()))
        o = buf.cpu().numpy()
        assert np.all(o[m:] == SENT), "rows >= m were written"
        assert not o[:m, f:].any(), "padding columns are not zero"
        return o[:m, :f], None
    Xd = _dev(_padded(X, ld))
    if mode in ("0", "4", "1-null") or (mode == "1" and not split):
        sc = {"0": 0, "4": 4}.get(mode, 1)
        out = torch.full((m + 2, ld), SENT, device="cuda")
        c0 = torch.full((m + TAIL,), SENT, device="cuda") if mode == "1" else None
        _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), sc, _ptr(out), _ptr(c0), _stream()))
        o = out.cpu().numpy()
        assert np.all(o[m:] == SENT), "rows >= m were written"
        assert not o[:m, f:].any(), "padding columns are not zero"
        if c0 is None:
            return o[:m, :f], None
        c = c0.cpu().numpy()
        assert np.all(c[m:] == SENT), "col0_out written behind row m"
        return o[:m, :f], c[:m]
    assert mode == "1" and split
    body = torch.full((m * (f - 1) + TAIL,), SENT, device="cuda")
    pairs = torch.full((2 * m + TAIL,), SENT, device="cuda")
    _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), 1, _ptr(body), _ptr(pairs), _stream()))
    b, p = body.cpu().numpy(), pairs.cpu().numpy()
    assert np.all(b[m * (f - 1):] == SENT) and np.all(p[2 * m:] == SENT), "written behind the packed body / the pairs"
    p = p[: 2 * m].reshape(m, 2)
    return np.concatenate([b[: m * (f - 1)].reshape(m, f - 1), p[:, :1]], axis=1), p[:, 1].copy()


def _check_refusals(X, W, ld):
    """Split layout: col0_out = NULL and out == in are refused with an error (and nothing is launched)."""
    _lib, lib, _ptr, _stream = _api()
    m, f = X.shape
    Xd, Wd = _dev(_padded(X, ld)), _dev(_padded(W, ld))
    body = torch.full((m * (f - 1) + TAIL,), SENT, device="cuda")
    pairs = torch.full((2 * m + TAIL,), SENT, device="cuda")
    with pytest.raises((ValueError, _lib.WmfLibraryError)):
        _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), 1, _ptr(body), None, _stream()))
    with pytest.raises((ValueError, _lib.WmfLibraryError)):
        _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), 1, _ptr(Xd), _ptr(pairs), _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Xd.cpu().numpy()), _bits(_padded(X, ld))) and bool((body == SENT).all()) and bool((pairs == SENT).all())


def _rolled_whitening(X, W, ld):
    """set_col0_one = 3 on X [m, 129]: returns (logical [m, f] result with the stuffed bits still in it, the raw packed body
    [m, f - 1], the pairs [m, 2])."""
    _lib, lib, _ptr, _stream = _api()
    m, f = X.shape
    Xd, Wd = _dev(_padded(X, ld)), _dev(_padded(W, ld))
    body = torch.full((m * (f - 1) + TAIL,), SENT, device="cuda")
    pairs = torch.full((2 * m + TAIL,), SENT, device="cuda")
    _lib.check(lib.wmf_row_transform(_ptr(Xd), m, f, ld, _ptr(Wd), 3, _ptr(body), _ptr(pairs), _stream()))
    b, p = body.cpu().numpy(), pairs.cpu().numpy()
    assert np.all(b[m * (f - 1):] == SENT) and np.all(p[2 * m:] == SENT), "written behind the packed body / the pairs"
    b, p = b[: m * (f - 1)].reshape(m, f - 1), p[: 2 * m].reshape(m, 2)
    # rolled by one: feature c at position c - 1, feature 0 last (the border feature of the pairs)
    return np.concatenate([p[:, :1], b], axis=1), b, p


def _check_rolled(got3, body3, pairs3, plain, X):
    """Mode 3 against the plain split-layout result `plain` (logical [m, f]) of the same call: equal, except that body positions
    8 j, 8 j + 1 (j < 16) may differ in their last mantissa bit only, and those 32 bits are the row's bias."""
    m, f = X.shape
    stuffed = np.zeros(f - 1, dtype=bool)
    pos = np.array([8 * j + b for j in range(16) for b in (0, 1)])
    stuffed[pos] = True
    a, b = _bits(body3), _bits(plain[:, 1:])
    assert np.array_equal(body3[:, ~stuffed], plain[:, 1:][:, ~stuffed])
    assert np.array_equal(a[:, stuffed] & ~np.uint32(1), b[:, stuffed] & ~np.uint32(1)), "more than the last mantissa bit moved"
    bias_bits = np.zeros(m, dtype=np.uint32)
    for j in range(16):
        for bb in (0, 1):
            bias_bits |= (a[:, 8 * j + bb] & np.uint32(1)) << np.uint32(2 * j + bb)
    assert np.array_equal(bias_bits, _bits(X[:, 0])), "the stuffed bits are not the row's bias"
    assert np.array_equal(_bits(pairs3[:, 1]), _bits(X[:, 0]))
    assert np.array_equal(pairs3[:, 0], plain[:, 0])
    assert np.all(pairs3[:, 0] == pairs3[0, 0]), "the border feature of the pairs differs between rows"


# ---------------------------------------------------------------------------------------------------------------- 1. Gramian
@pytest.mark.parametrize("f,bias,flags", GRAM_CASES)
def test_gramian_is_exact_on_small_integers(f, bias, flags):
    """1a / 1d.  Integer entries in [-7, 7]: every product and every partial sum is an integer below 2^24 and the cross-wave
    sum is float64, so G must EQUAL the float64 reference at every row count -- the row masks of ragged chunks, the clamped
    loads, col_mask_last, the bias column, the tile -> matrix scatter of both reduce kernels, the symmetric fill.  Two calls
    are bit-identical."""
    _lib, lib, _ptr, _stream = _api()
    with _flags(lib, flags):
        ms = M_EDGES + ((_big_m(f),) if _big_m(f) else ())
        for m in ms:
            Y = _integers(m, f, seed=7 * f + m)
            g1, g2 = _gram(Y, bias, calls=2)
            Yt = _tilde(Y, bias)
            Gref = Yt.T @ Yt
            bad = np.argwhere(g1 != Gref)
            assert not len(bad), (f, bias, m, len(bad), bad[:4].tolist(), [(g1[i, j], Gref[i, j]) for i, j in bad[:4]])
            assert np.array_equal(g1, g2)


@pytest.mark.parametrize("f,bias,flags", GRAM_CASES)
def test_gramian_few_terms_per_element(f, bias, flags):
    """1b.  m in {1, 4, 8} rows of graded columns.  Per element |G_ij - Gref_ij| <= 2 (m + 2) u (|Y|^T |Y|)_ij: m u is the
    bound of an m-term float32 dot product in any order, one u for the dropped products of the bf16 split ("below 2^-24 of
    the term"), one for the final rounding, doubled to admit an accumulator that truncates.  Float32 arithmetic needs
    1 .. 3.4 u here, the six-product split below 1 u, a split with any one product left out >= 100 u (CPU emulation at
    f = 129, 20 draws): the gate of 6 / 12 / 20 u has a factor of five on both sides."""
    _lib, lib, _ptr, _stream = _api()
    worst = {}
    with _flags(lib, flags):
        for m in (1, 4, 8):
            for draw in range(4):
                Y = _graded(m, f, seed=31 * f + 5 * m + draw)
                (G,) = _gram(Y, bias)
                Yt = _tilde(Y, bias)
                Gref, mag = Yt.T @ Yt, np.abs(Yt).T @ np.abs(Yt)
                assert np.all(mag > 0)
                ratio = np.abs(G - Gref) / (mag * U)
                worst[m] = max(worst.get(m, 0.0), float(ratio.max()))
                i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
                assert ratio.max() <= 2 * (m + 2), (f, bias, m, draw, (int(i), int(j)), float(ratio.max()), G[i, j], Gref[i, j])
    record_error(f"dense_gram_few_terms[f={f},bias={bias},flags={flags}]", **{f"u_m{m}": v for m, v in worst.items()})


def _scaled_error(G, Gref):
    d = np.sqrt(np.diag(Gref))
    return float((np.abs(G - Gref) / np.outer(d, d)).max())


@pytest.mark.parametrize("f,bias,flags", GRAM_CASES)
def test_gramian_scaled_error_against_numpy_float32(f, bias, flags):
    """1c / 1d.  Full length (m = 1234 and, for one width per block count, a count beyond the rounding of the wave count), graded
    columns.  Cholesky and the whitening are invariant under column scaling; what they amplify is
    e = max_ij |dG_ij| / sqrt(G_ii G_jj).  Gate: e of the device <= e of NumPy's float32 product of the same input, measured
    here, no margin -- the kernels carry at most a few thousand rows per float32 accumulator before the float64 reduction,
    NumPy's product carries all of them in float32."""
    _lib, lib, _ptr, _stream = _api()
    with _flags(lib, flags):
        for m in (1234,) + ((_big_m(f),) if _big_m(f) else ()):
            Y = _graded(m, f, seed=13 * f + 1)
            g1, g2 = _gram(Y, bias, calls=2)
            assert np.array_equal(g1, g2)
            Yt = _tilde(Y, bias)
            Gref = Yt.T @ Yt
            Y32 = _tilde(Y, bias, np.float32)
            e_dev, e_np = _scaled_error(g1, Gref), _scaled_error((Y32.T @ Y32).astype(np.float64), Gref)
            record_error(f"dense_gram_scaled[f={f},bias={bias},flags={flags},m={m}]", device=e_dev, numpy32=e_np)
            print(f"gram scaled f={f} bias={bias} flags={flags} m={m}: device {e_dev:.3e} numpy32 {e_np:.3e}")
            assert np.array_equal(g1, g1.T)
            assert e_dev <= e_np, (f, bias, flags, m, e_dev, e_np)


@pytest.mark.parametrize("f", WIDTHS)
def test_gramian_of_no_rows_and_workspace_bounds(f):
    """1e.  m = 0 gives a zero matrix; gram + factorize leave the bytes behind wmf_gram_workspace_bytes(f) alone."""
    _lib, lib, _ptr, _stream = _api()
    (G0,) = _gram(np.zeros((0, f), dtype=np.float32), 0)
    assert G0.shape == (f, f) and not G0.any()
    ld, m = lib.wmf_ld_for(f), 1234
    nbytes = int(lib.wmf_gram_workspace_bytes(f))
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    Yd = _dev(_padded(_graded(m, f, seed=f), ld))
    G = torch.zeros(f * f, dtype=torch.float64, device="cuda")
    Ww, Wu = torch.zeros(f, ld, device="cuda"), torch.zeros(f, ld, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_gram(_ptr(Yd), m, f, ld, 1, _ptr(G), _ptr(ws), _stream()))
    _lib.check(lib.wmf_factorize(_ptr(G), f, ld, 0.1, _ptr(Ww), _ptr(Wu), _ptr(info), _ptr(ws), _stream()))
    assert int(info[0]) == 0
    assert bool((ws[nbytes:] == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------- 2. factorisation
def _gaussian_gramian(f):
    Y = np.random.default_rng(50_000 + f).standard_normal((1234, f))
    return Y.T @ Y


def _graded_gramian(f):
    Y = _graded(1234, f, seed=60_000 + f).astype(np.float64)
    return Y.T @ Y


C_F = 8                                                           # c_f = 8 f: the float64 part of the bound below


@pytest.mark.parametrize("case", ["gaussian", "graded"])
@pytest.mark.parametrize("f", range(1, WMF_MAX_F + 1))
def test_factorisation_per_element_at_every_width(f, case):
    """Every f = 1 .. 260 (every block count and ragged last block of both kernels), A = G + 0.1 I from a well-conditioned
    Gaussian Gramian and from the graded-column one (condition 1e5 .. 1e8).  Per element
        |W_unwhite - L^-1| <= u |L^-1| + 8 f cond2(A) 2^-53 max|L^-1|
    -- one float32 rounding of a float64 result plus the forward-error bound of Cholesky and triangular inversion in
    float64 (NumPy's own L^-1, checked against an np.longdouble Cholesky and inversion at every ninth width of both cases,
    needs at most 0.37 f cond2(A) 2^-53 max|L^-1|: c_f = 8 f stands).
    W_white is the bitwise transpose, both are exactly zero outside their triangle and in the padding columns, info stays
    0.  Gaussian case: max |W A W^T - I| <= f 2^-21 in float64 (each entry of W carries one float32 rounding; the float32
    rounding of NumPy's own L^-1 needs at most 0.04 of that)."""
    G = _gaussian_gramian(f) if case == "gaussian" else _graded_gramian(f)
    lam = 0.1
    Ww, Wu, info = _factorize(G, lam)
    assert int(info[0]) == 0
    A = G + lam * np.eye(f)
    Linv = np.linalg.inv(np.linalg.cholesky(A))
    cond = np.linalg.cond(A)
    bound = U * np.abs(Linv) + C_F * f * cond * 2.0 ** -53 * np.abs(Linv).max()
    err = np.abs(Wu[:, :f].astype(np.float64) - Linv)
    k = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (f, case, k, err[k], bound[k], cond)
    assert np.array_equal(_bits(Ww[:, :f]), _bits(Wu[:, :f].T)), "W_white is not the bitwise transpose of W_unwhite"
    assert not np.triu(Wu[:, :f], 1).any() and not np.tril(Ww[:, :f], -1).any()
    assert not Wu[:, f:].any() and not Ww[:, f:].any()
    if case == "gaussian":
        W = Wu[:, :f].astype(np.float64)
        res = float(np.abs(W @ A @ W.T - np.eye(f)).max())
        assert res <= f * 2.0 ** -21, (f, res, f * 2.0 ** -21)


@pytest.mark.parametrize("f", [8, 64, 65, 129, 200, 260])
def test_factorisation_reports_the_failing_leading_minor(f):
    """A positive definite A with A[j-1, j-1] negated: leading minor j is the first that is not positive definite, and
    info[0] == j is what include/wmf_hip.h documents.  Both outputs are zero matrices, and a following successful call leaves
    info as it was (sticky)."""
    A0 = _gaussian_gramian(f) + 0.1 * np.eye(f)
    ran = 0
    minors = sorted(j for j in {1, 16, 17, 64, 65, f} if j <= f)
    for j in minors:
        A = A0.copy()
        A[j - 1, j - 1] = -A[j - 1, j - 1]
        Ww, Wu, info = _factorize(A, 0.0)
        assert int(info[0]) == j, (f, j, int(info[0]))
        assert not Ww.any() and not Wu.any()
        Ww, Wu, info = _factorize(A0, 0.0, info=info)             # success after failure: the flag stays
        assert int(info[0]) == j and Wu[:, :f].any()
        ran += 1
    assert ran == len(minors) >= 2


# ----------------------------------------------------------------------------------------------------------- 3. row transform
def _signed_permutation(f, seed, fix0=False):
    """W[k, pi(k)] = +- 2^s, |s| <= 3 (fix0: pi(0) = 0, so that with a column of ones whitened feature 0 is one number)."""
    rng = np.random.default_rng(seed)
    pi = rng.permutation(f)
    if fix0:
        pi = np.concatenate([[0], 1 + rng.permutation(f - 1)])
    val = (rng.choice([-1.0, 1.0], f) * 2.0 ** rng.integers(-3, 4, f)).astype(np.float32)
    W = np.zeros((f, f), dtype=np.float32)
    W[np.arange(f), pi] = val
    return W, pi, val


@pytest.mark.parametrize("f", WIDTHS)
def test_transform_is_exact_for_signed_permutations(f):
    """3a / 3e.  W a signed, power-of-two-scaled permutation: out[r, pi(k)] = +- 2^s in~[r, k] EXACTLY, on every path -- also
    through the split-bf16 kernel, whose three bf16 parts of a float32 recombine exactly.  Every mode the width supports
    (out != in, in place, column 0 read as one with and without the bias copy, the split layout and its refusals, the rolled
    modes), every row count, the layouts' own promises (zero padding, nothing written behind an array, bias bitwise), two runs
    bit-identical.  The number of modes run is the number the ABI's predicates enumerate."""
    _lib, lib, _ptr, _stream = _api()
    ld = lib.wmf_ld_for(f)
    expected = _modes_of(lib, f, ld)
    assert ("1-refusals" in expected) == (f in SPLIT_WIDTHS) and (("3" in expected) == (f == 129))
    ran = []
    for mode in expected:
        W, pi, val = _signed_permutation(f, seed=3 * f + len(ran), fix0=(mode == "3"))
        for m in M_EDGES:
            X = _graded(m, f, seed=17 * f + m)
            one = mode in ("1", "1-null", "3")
            Xt = _tilde(X, one, np.float32)
            ref = np.zeros((m, f), dtype=np.float32)
            ref[:, pi] = Xt * val[None, :]
            if mode == "1-refusals":
                _check_refusals(X, W, ld)
                continue
            if mode == "3":
                got3, body3, pairs3 = _rolled_whitening(X, W, ld)
                plain, _ = _transform(X, W, "1", ld)
                assert np.array_equal(plain, ref)
                _check_rolled(got3, body3, pairs3, plain, X)
                if m == 1234:
                    again = _rolled_whitening(X, W, ld)
                    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((got3, body3, pairs3), again))
                continue
            got, c0 = _transform(X, W, mode, ld)
            bad = np.argwhere(got != ref)
            assert not len(bad), (f, mode, m, len(bad), bad[:4].tolist(), [(got[i, j], ref[i, j]) for i, j in bad[:4]])
            if mode == "1":
                assert np.array_equal(_bits(c0), _bits(X[:, 0]))
            if m == 1234:
                got2, c02 = _transform(X, W, mode, ld)
                assert np.array_equal(_bits(got), _bits(got2)) and (c0 is None or np.array_equal(_bits(c0), _bits(c02)))
        ran.append(mode)
    assert ran == expected and len(ran) == 4 + 2 * (f == 129)


def _banded(f, seed):
    """Upper band of width 4 of random 24-bit values: every output is a dot product of at most four terms."""
    rng = np.random.default_rng(seed)
    W = np.zeros((f, f), dtype=np.float32)
    for d in range(min(4, f)):
        k = np.arange(f - d)
        W[k, k + d] = (rng.integers(-2 ** 23, 2 ** 23, f - d) / 2.0 ** 23).astype(np.float32)
    return W


@pytest.mark.parametrize("f", WIDTHS)
def test_transform_few_terms_per_element(f):
    """3b.  Banded W: |out - ref| <= 2 (4 + 2) u (|in~| |W|) per element, the derivation of the Gramian's few-term gate.  Sees a
    lost product of the split kernels (>= 100 u) on every path that multiplies: out != in, in place, column 0 as one (split
    layout where the width has it) and the rolled input."""
    _lib, lib, _ptr, _stream = _api()
    ld = lib.wmf_ld_for(f)
    modes = [md for md in _modes_of(lib, f, ld) if md in ("0", "0-in-place", "1", "4")]
    W = _banded(f, seed=9 * f)
    worst, ran = 0.0, 0
    for mode in modes:
        for m in (33, 1234):
            X = _graded(m, f, seed=19 * f + m)
            Xt = _tilde(X, mode == "1")
            ref, mag = Xt @ W.astype(np.float64), np.abs(Xt) @ np.abs(W).astype(np.float64)
            got, _ = _transform(X, W, mode, ld)
            ratio = np.abs(got - ref) / np.where(mag > 0, mag * U, 1.0)
            assert np.all(got[mag == 0] == 0)
            worst = max(worst, float(ratio.max()))
            k = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert ratio.max() <= 2 * (4 + 2), (f, mode, m, k, float(ratio.max()), got[k], ref[k])
            ran += 1
    assert ran == 2 * (3 + (f == 129))
    record_error(f"dense_transform_few_terms[f={f}]", u=worst)


# The margin of 3c.  At x 1 the f32-MFMA transform misses NumPy's figure at most narrow widths (f = 16 with biases: 6.2 u against
# 2.3 u; 2.7 x is the worst of the 104 cases, the split-bf16 kernel of f = 97 .. 144 needs at most 1.2 x) without being wrong:
# NumPy -- its sgemm and a plain sequential float32 loop alike, 2.3 u both -- rounds every addition to nearest, so its n errors
# of at most u cancel; a v_mfma_f32_16x16x4_f32 step adds four products and the accumulator in one operation that is not
# specified to round each addition to nearest (four-term Gramian entries sit at 3.3 u where one-term entries sit at 1.0 u).
# Two factors of 2: one ulp = 2 u per step for an accumulator that truncates (what the few-term gates admit), and the sum of
# two such one-sided errors per four-product step where NumPy's signs cancel.  A truncating float32 accumulator restated in
# NumPy gives 5 .. 170 u on the same operands (linear in f): the device is far inside that, and every case records both figures.
WHITENING_MARGIN = 4


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", WIDTHS)
def test_whitening_dense_against_numpy_float32(f, bias):
    """3c.  The real whitening: the graded factors times the W_white the device factorised from their Gramian (lambda = 0.1).
    Per element |out - ref| / (|in~| |W|), gate = WHITENING_MARGIN x the same quantity for NumPy's float32 product of the same
    operands, measured here: both sum f <= 260 terms in float32."""
    _lib, lib, _ptr, _stream = _api()
    ld, m = lib.wmf_ld_for(f), 1234
    Y = _graded(m, f, seed=23 * f + bias)
    Yt = _tilde(Y, bias)
    Ww, Wu, info = _factorize(Yt.T @ Yt, 0.1, ld)
    assert int(info[0]) == 0
    W = Ww[:, :f]
    got, c0 = _transform(Y, W, "1" if bias else "0", ld)
    got2, _ = _transform(Y, W, "1" if bias else "0", ld)
    assert np.array_equal(_bits(got), _bits(got2))
    ref, mag = Yt @ W.astype(np.float64), np.abs(Yt) @ np.abs(W).astype(np.float64)
    np32 = _tilde(Y, bias, np.float32) @ W
    e_dev, e_np = float((np.abs(got - ref) / mag).max()), float((np.abs(np32 - ref) / mag).max())
    record_error(f"dense_whitening[f={f},bias={bias}]", device=e_dev, numpy32=e_np)
    print(f"whitening f={f} bias={bias}: device {e_dev / U:.2f} u numpy32 {e_np / U:.2f} u")
    if bias:
        assert np.array_equal(_bits(c0), _bits(Y[:, 0]))
    assert e_dev <= WHITENING_MARGIN * e_np, (f, bias, e_dev, e_np)


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", WIDTHS)
def test_three_passes_whiten_to_the_identity(f, bias):
    """3d.  gram -> factorize -> transform, all on the device, well-conditioned factors: V^T V + lambda W^T W is the identity
    to f 2^-20 in float64 -- the three passes tied together at every block count."""
    _lib, lib, _ptr, _stream = _api()
    ld, m, lam = lib.wmf_ld_for(f), 1234, 0.1
    Y = np.random.default_rng(70_000 + f).standard_normal((m, f), dtype=np.float32)
    (G,) = _gram(Y, bias, ld)
    Ww, Wu, info = _factorize(G, lam, ld)
    assert int(info[0]) == 0
    V, _ = _transform(Y, Ww[:, :f], "1" if bias else "0", ld)
    V, W = V.astype(np.float64), Ww[:, :f].astype(np.float64)
    res = float(np.abs(V.T @ V + lam * W.T @ W - np.eye(f)).max())
    record_error(f"dense_whiten_identity[f={f},bias={bias}]", residual=res, gate=f * 2.0 ** -20)
    assert res <= f * 2.0 ** -20, (f, bias, res)


def test_rolled_whitening_of_the_real_factors():
    """Modes 3 and 4 at f = 129 on the real thing (W_white / W_unwhite of the graded factors, every row count): mode 3 is the
    plain split-layout whitening rolled by one position, bias bits in the last mantissa bit of positions 8 j, 8 j + 1, the
    border feature one number for all rows; mode 4 un-whitens a rolled g within the few-term gate's per-element form of the
    dense bound ((f + 2) u, doubled) -- it sums the same products as mode 0 in another order."""
    _lib, lib, _ptr, _stream = _api()
    f = 129
    ld = lib.wmf_ld_for(f)
    assert lib.wmf_rolled_layout_supported(f, ld)
    Yall = _graded(1234, f, seed=4242)
    Yt = _tilde(Yall, 1)
    Ww, Wu, info = _factorize(Yt.T @ Yt, 0.1, ld)
    assert int(info[0]) == 0
    for m in M_EDGES:
        X = Yall[:m]
        plain, _ = _transform(X, Ww[:, :f], "1", ld)
        got3, body3, pairs3 = _rolled_whitening(X, Ww[:, :f], ld)
        _check_rolled(got3, body3, pairs3, plain, X)
        g = plain                                                 # any [m, f] block serves as the g of the un-whitening
        out4, _ = _transform(g, Wu[:, :f], "4", ld)
        ref = g.astype(np.float64) @ Wu[:, :f].astype(np.float64)
        mag = np.abs(g).astype(np.float64) @ np.abs(Wu[:, :f]).astype(np.float64)
        assert np.all(np.abs(out4 - ref) <= 2 * (f + 2) * U * mag)
