"""The reversed whitening of the chained path in NumPy float64 ("One whitening reversed"; include/wmf_hip.h,
WMF_COMPOSE_REVERSED): no GPU.

Any W = P L^-T with L L^T = P^T A P whitens A.  The users' side takes P = diag(1, J) (bias; J reverses features 1 .. f - 1) or
P = J (no bias), the items' side P = I.  N = T . W_white of either side is then a product of one reversed and one plain
triangular matrix, and N[i][j] = 0 exactly for i + j < f (bias; i + j < f - 1 without), where a plain pair gives a dense N.
The tile counts are those of chain6_kernel: 32-wide K chunks x 16-wide output blocks of N_ext in the kernel's positions."""
import numpy as np
import pytest

LAM = 0.1
WIDTHS = [(f, b) for f in (97, 113, 129) for b in (0, 1)]


def perm(f, bias, rev):
    """wmf_perm of csrc/wmf_dense.hip as an index vector."""
    j = np.arange(f)
    if not rev:
        return j
    return np.where(j == 0, 0, f - j) if bias else f - 1 - j


def inv_lower(L):
    """L^-1 by forward substitution: the zeros above the diagonal are exact (a general inverse may pivot)."""
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        e = np.zeros(i + 1)
        e[i] = 1.0
        X[i, : i + 1] = (e - L[i, :i] @ X[:i, : i + 1]) / L[i, i]
    return X


def whitening(A, bias, rev):
    """(W_white, W_unwhite) in feature order: P L^-T and L^-1 P^T with L = chol(P^T A P)."""
    p = perm(A.shape[0], bias, rev)
    Linv = inv_lower(np.linalg.cholesky(A[np.ix_(p, p)]))
    Wu = Linv[:, p]                                               # (p is an involution)
    return Wu.T.copy(), Wu


def t_matrix(U, bias):
    T = U.copy()
    if bias:
        T[:, 0] = 0
        T = np.concatenate([T, np.eye(1, U.shape[0])], axis=0)
    return T


def n_ext(U, Ww, bias):
    """[T . W_white | U[:, 0]]: (f + bias) x (f + bias), feature order."""
    N = t_matrix(U, bias) @ Ww
    if bias:
        N = np.concatenate([N, np.concatenate([U[:, :1], np.zeros((1, 1))])], axis=1)
    return N


def spd(f, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((4 * f, f)) * 2.0 ** rng.integers(-4, 2, (1, f))
    return Y.T @ Y + LAM * np.eye(f)


def live_pairs(N, f, bias, rolled, short_tail):
    """Tile pairs chain6_kernel issues for N_ext (feature order in, positions inside)."""
    f1 = f + bias
    pos = np.concatenate([(np.arange(f) + 1) % f, np.arange(f, f1)]) if rolled else np.arange(f1)
    Np = N[np.ix_(pos, pos)]
    nfb = (f1 + 15) // 16
    nkc = (16 * nfb + 31) // 32
    P = np.zeros((32 * nkc, 16 * nfb))
    P[:f1, :f1] = Np
    live = (P.reshape(nkc, 32, nfb, 16) != 0).any(axis=(1, 3))
    if short_tail and f1 - 32 * (nkc - 1) <= 2:
        live = live[:-1]
    return int(live.sum())


def chain(f, bias, reverse_users):
    """Three consecutive whitenings items -> users -> items and the two N_ext between them."""
    Wi, Ui = whitening(spd(f, 10 * f + bias), bias, False)             # the items' whitening un-whitens the users' g
    Wu, Uu = whitening(spd(f, 10 * f + bias + 1), bias, reverse_users)
    Wi2, _ = whitening(spd(f, 10 * f + bias + 2), bias, False)
    return (Wu, Uu), n_ext(Ui, Wu, bias), n_ext(Uu, Wi2, bias)


@pytest.mark.parametrize("f,bias", WIDTHS)
def test_reversed_whitening_is_a_whitening(f, bias):
    A = spd(f, 7 * f + bias)
    W, Uw = whitening(A, bias, True)
    assert np.abs(W.T @ A @ W - np.eye(f)).max() <= 1e-9
    assert np.array_equal(Uw, W.T)
    # anti-triangular in feature order, the border feature apart
    i, j = np.indices((f, f))
    zero = (i + j < f) & (i >= 1) & (j >= 1) | (i >= 1) & (j == 0) if bias else (i + j < f - 1)
    assert not W[zero].any()
    if bias:
        # the whitened border feature is the constant 1 / L00 on every row of in~ = [1, x_1 .. x_{f-1}]
        rng = np.random.default_rng(f)
        X = np.concatenate([np.ones((50, 1)), rng.standard_normal((50, f - 1))], axis=1)
        V = X @ W
        assert np.ptp(V[:, 0]) == 0 and abs(V[0, 0] - 1 / np.sqrt(A[0, 0])) <= 1e-12


@pytest.mark.parametrize("f,bias", WIDTHS)
def test_n_ext_zeros_are_exact_on_both_sides(f, bias):
    _, Nu, Ni = chain(f, bias, True)
    f1 = f + bias
    i, j = np.indices((f1, f1))
    predicted = (i + j < f) if bias else (i + j < f - 1)
    for N in (Nu, Ni):
        assert not N[predicted].any()                             # exactly zero: sums of exact zeros
        assert N[1:f, 1:f][~predicted[1:f, 1:f]].all()            # and nothing else is
    if bias:
        # V[:, 0] of a chained pass: only the row of the one reaches column 0
        g = np.random.default_rng(3).standard_normal((40, f))
        V = np.concatenate([g, np.ones((40, 1))], axis=1) @ Nu
        assert np.ptp(V[:, 0]) == 0 and V[0, 0] == Nu[f, 0] != 0
    # the plain pair: dense
    _, Nd, _ = chain(f, bias, False)
    assert np.count_nonzero(Nd[1:f, 1:f]) == (f - 1) ** 2


def test_live_tile_pairs_at_the_flagship_width():
    f, bias = 129, 1
    _, Nd, _ = chain(f, bias, False)
    _, Nu, Ni = chain(f, bias, True)
    assert live_pairs(Nd, f, bias, True, False) == 45
    for N in (Nu, Ni):
        assert live_pairs(N, f, bias, True, False) == 33
        assert live_pairs(N, f, bias, True, True) == 24
        # K chunks 0 .. 3 keep 3, 5, 7 and 9 blocks, chunk 4 keeps 9
        pos = np.concatenate([(np.arange(f) + 1) % f, [f]])
        P = np.zeros((160, 144))
        P[:130, :130] = N[np.ix_(pos, pos)]
        assert (P.reshape(5, 32, 9, 16) != 0).any(axis=(1, 3)).sum(axis=1).tolist() == [3, 5, 7, 9, 9]
    assert live_pairs(Nd, f, bias, True, True) == 36               # the short last chunk alone, on a dense N_ext


@pytest.mark.parametrize("f,bias", WIDTHS)
def test_live_tile_pairs_drop_at_every_width(f, bias):
    _, Nd, _ = chain(f, bias, False)
    _, Nu, Ni = chain(f, bias, True)
    f1 = f + bias
    nfb = (f1 + 15) // 16
    nkc = (16 * nfb + 31) // 32
    for rolled in ((0, 1) if (f, bias) == (129, 1) else (0,)):
        dense = live_pairs(Nd, f, bias, rolled, False)
        assert dense == nfb * nkc
        for N in (Nu, Ni):
            assert live_pairs(N, f, bias, rolled, True) <= live_pairs(N, f, bias, rolled, False) < dense
