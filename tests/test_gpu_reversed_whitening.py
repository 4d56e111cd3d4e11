"""The reversed whitening of the chained path on the device ("One whitening reversed"; include/wmf_hip.h,
WMF_COMPOSE_REVERSED) and the short last K chunk of chain6_kernel.

    wmf_compose_whitening(rolled | 2)   P^T (G~ + lambda I) P = L L^T; W_white = P L^-T, W_unwhite = L^-1 P^T in feature order
    wmf_row_transform_chained           a . N_ext for an anti-triangular and for a dense N_ext; where the last K chunk holds one
                                        or two live positions (f + bias = 97, 98, 129, 130) the accumulators start from them
    AlsEngine                           the users' whitening reversed, the items' not

The helpers and the bounds are those of tests/test_gpu_chained.py (copied: a test module is not imported): per element
2 (n + 2) u sum |x| |y| for the chained pass, the factorisation gate u |L^-1| + 8 f cond2(A) 2^-53 max |L^-1|, the compose gate
u |ref| + f 2^-52 sum |T| |W|.  The identity W_unwhite A W_white = I is checked with that factorisation gate carried through the
product: |E| |A W| + |U A| |E|^T for an error E within the gate (A W = P L, so the bound is of the size of u cond(L))."""
import numpy as np
import pytest
import torch

from conftest import record_error
from oracle import wmf_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_F = 8
SENT = 3.0
REVERSED = 2
CASES = [(f, b) for f in (97, 113, 128, 129, 144) for b in (0, 1) if f + b <= min(144, (f + 3) & ~3)]
assert len(CASES) == 8
M_EDGES = (1, 15, 16, 17, 31, 32, 33, 127, 129, 161)
# the chained pass: f1 = 97, 98, 129, 130 start the accumulators from the last chunk; 113, 114: the MFMA path kept (17, 18 live
# positions in the last chunk); 128: the last chunk does not exist
PASS_WIDTHS = [(97, 0), (97, 1), (113, 0), (113, 1), (128, 0), (129, 0), (129, 1)]


def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _column_scales(f, seed):
    rng = np.random.default_rng(1000 + seed)
    return (2.0 ** rng.permutation(np.resize(np.arange(-10, 3), f))).astype(np.float32)


_BASE = np.random.default_rng(99).standard_normal((200, 160), dtype=np.float32)


def _g_rows(m, f, seed):
    return np.ascontiguousarray(_BASE[:m, :f] * _column_scales(f, seed)[None, :])


def _padded_nan(g, ld, extra_rows=2):
    m, f = g.shape
    P = np.full((m + extra_rows, ld), np.nan, dtype=np.float32)
    P[:m, :f] = g
    return P


def _aug(g, bias):
    a = g.astype(np.float64)
    return np.concatenate([a, np.ones((a.shape[0], 1))], axis=1) if bias else a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ws(lib, f):
    return torch.empty(int(lib.wmf_gram_workspace_bytes(f + 1)), dtype=torch.uint8, device="cuda")


def _perm(f, bias):
    j = np.arange(f)
    return np.where(j == 0, 0, f - j) if bias else f - 1 - j


def _positions(f, f1, rolled):
    """Feature (f: the one / the bias column) at each position of a row of g and of N_ext."""
    return np.concatenate([(np.arange(f) + 1) % f, np.arange(f, f1)]) if rolled else np.arange(f1)


def _predicted_zero(f, bias, rolled):
    """[f1, f1] mask in positions: N_ext[i][j] = 0 for i + j < f in feature indices (i + j < f - 1 without biases)."""
    f1 = f + bias
    pos = _positions(f, f1, rolled)
    i, j = pos[:, None], pos[None, :]
    return (i + j < f) if bias else (i + j < f - 1)


# ------------------------------------------------------------------------------------------------------- 1. compose
def _t_matrix(Uw, f, bias, rolled):
    src = (np.arange(f) + 1) % f if rolled else np.arange(f)
    T = Uw[src].astype(np.float64)
    if bias:
        T[:, 0] = 0
        T = np.concatenate([T, np.eye(1, f)], axis=0)
    return T


def _compose(Gaug, Uw, f, ld, bias, flags, lam):
    _lib, lib, _ptr, _stream = _api()
    f1 = f + bias
    Ud = torch.zeros(f, ld, device="cuda")
    Ud[:, :f] = _dev(Uw)
    Ww, Wu, N = (torch.full((r, ld), 7.0, device="cuda") for r in (f, f, f1))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_compose_whitening(_ptr(_dev(Gaug.reshape(-1))), _ptr(Ud), f, ld, bias, int(flags), lam, _ptr(Ww), _ptr(Wu),
                                         _ptr(N), _ptr(info), _ptr(_ws(lib, f)), _stream()))
    return Ww.cpu().numpy(), Wu.cpu().numpy(), N.cpu().numpy(), int(info[0])


def _check_n_ext(N, Uw, Ww, f, bias, rolled):
    """N_ext against float64 [T . W_white | U[:, 0]] from the float32 W_white the call returned (the compose gate)."""
    f1 = f + bias
    T = _t_matrix(Uw, f, bias, rolled)
    col = (np.arange(f) + 1) % f if rolled else np.arange(f)
    W64 = Ww[:, :f].astype(np.float64)[:, col]
    ref, mag = T @ W64, np.abs(T) @ np.abs(W64)
    assert np.all(np.abs(N[:, :f] - ref) <= U * np.abs(ref) + f * 2.0 ** -52 * mag)
    if bias:
        src = (np.arange(f) + 1) % f if rolled else np.arange(f)
        assert np.array_equal(_bits(N[:f, f]), _bits(Uw[src, 0])) and N[f, f] == 0
    assert not N[:, f1:].any()


@pytest.mark.parametrize("f,bias,rolled", [(f, b, 0) for f, b in CASES] + [(129, 1, 1)])
def test_compose_reversed(f, bias, rolled):
    _lib, lib, _ptr, _stream = _api()
    ld, f1, lam = lib.wmf_ld_for(f), f + bias, 0.1
    rng = np.random.default_rng(9000 + f + bias)
    Y = rng.standard_normal((600, f))
    Uw = np.linalg.inv(np.linalg.cholesky(Y.T @ Y + lam * np.eye(f))).astype(np.float32)
    Uw = np.tril(Uw)                                              # (the engine's: exact zeros above the diagonal)
    a = _aug(_g_rows(150, f, seed=f) * np.float32(8.0), bias)
    Gaug = a.T @ a
    plain = _compose(Gaug, Uw, f, ld, bias, rolled, lam)
    again = _compose(Gaug, Uw, f, ld, bias, rolled, lam)
    assert plain[3] == 0
    for x, y in zip(plain[:3], again[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.triu(plain[1][:, :f], 1).any()                  # flag off: W_unwhite = L^-1, lower triangular as ever
    Ww, Wu, N, info = _compose(Gaug, Uw, f, ld, bias, rolled | REVERSED, lam)
    assert info == 0
    T = _t_matrix(Uw, f, bias, rolled)
    A = T.T @ Gaug @ T + lam * np.eye(f)
    p = _perm(f, bias)
    Linv, cond = np.linalg.inv(np.linalg.cholesky(A[np.ix_(p, p)])), np.linalg.cond(A)
    Linv = np.tril(Linv)
    ref = Linv[:, p]                                              # L^-1 P^T
    bound = U * np.abs(ref) + C_F * f * cond * 2.0 ** -53 * np.abs(Linv).max()
    err = np.abs(Wu[:, :f].astype(np.float64) - ref)
    k = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (f, bias, k, err[k], bound[k], cond)
    assert np.array_equal(_bits(Ww[:, :f]), _bits(Wu[:, :f].T))
    assert not Wu[:, f:].any() and not Ww[:, f:].any()
    # the zeros of L^-1 arrive as zeros: anti-triangular in feature order
    assert not Wu[:, :f][ref == 0].any() and (ref == 0).sum() == f * (f - 1) // 2
    # W_unwhite A W_white = I (and so W_white^T A W_white = I: the same bits transposed), the gate carried through the product
    Wu64, Ww64 = Wu[:, :f].astype(np.float64), Ww[:, :f].astype(np.float64)
    resid = np.abs(Wu64 @ A @ Ww64 - np.eye(f))
    rb = bound @ np.abs(A @ ref.T) + np.abs(ref @ A) @ bound.T
    rb = 1.01 * rb + f * 2.0 ** -50 * (np.abs(ref) @ np.abs(A) @ np.abs(ref.T))
    assert np.all(resid <= rb), (f, bias, float((resid / rb).max()))
    assert np.all(np.abs(Ww64.T @ A @ Ww64 - np.eye(f)) <= rb)
    worst_gate = float((err / bound).max())
    # N_ext: the compose gate, and the predicted zeros exactly zero (U plain, W_white reversed)
    _check_n_ext(N, Uw, Ww, f, bias, rolled)
    zero = _predicted_zero(f, bias, rolled)
    assert not N[:, :f1][zero].any()
    assert N[:, :f1][~zero].astype(bool).sum() >= (~zero).sum() - f1 - 1          # (nothing else: N[f][f] and row 0's column apart)
    # ... and the next half step's: U reversed (the W_unwhite just returned), W_white plain
    Ww2, Wu2, N2, info2 = _compose(Gaug, Wu[:, :f], f, ld, bias, rolled, lam)
    assert info2 == 0 and not np.triu(Wu2[:, :f], 1).any()
    _check_n_ext(N2, Wu[:, :f], Ww2, f, bias, rolled)
    assert not N2[:, :f1][zero].any()
    # flag on and off are different whitenings of the same matrix
    assert not np.array_equal(_bits(plain[1]), _bits(Wu))
    # not positive definite: info names the minor, the outputs are zero matrices
    Ww, Wu, N, info = _compose(-Gaug - np.eye(f1), Uw, f, ld, bias, rolled | REVERSED, lam)
    assert info >= 1 and not Ww.any() and not Wu.any() and not N[:, :f].any()
    record_error(f"reversed_compose[f={f},bias={bias},rolled={rolled}]", worst_of_gate=worst_gate,
                 worst_identity_of_bound=float((resid / rb).max()))


def test_compose_rejects_unknown_flags():
    _lib, lib, _ptr, _stream = _api()
    f, bias = 129, 1
    ld = lib.wmf_ld_for(f)
    t = torch.zeros(131 * 132, dtype=torch.float64, device="cuda")
    w = [torch.zeros(131, ld, device="cuda") for _ in range(4)]
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.wmf_compose_whitening(_ptr(t), _ptr(w[0]), f, ld, bias, 4, 0.1, _ptr(w[1]), _ptr(w[2]), _ptr(w[3]), _ptr(info),
                                     _ptr(_ws(lib, f)), _stream()) != 0


# ------------------------------------------------------------------------------------------------------- 2. the chained pass
def _chained(g, N, bias, rolled, ld):
    _lib, lib, _ptr, _stream = _api()
    m, f = g.shape
    f1 = f + bias
    gd = _dev(_padded_nan(g, ld))
    Nd = torch.zeros(f1, ld, device="cuda")
    Nd[:, :f1] = _dev(N.astype(np.float32))
    ldv = lib.wmf_whitened_row_floats(f, ld, bias)
    split = bool(bias) and ldv == f - 1
    assert split or not rolled
    body = torch.full(((m + 2) * ldv,), SENT, device="cuda")
    pairs = torch.full(((m + 2) * (2 if split else 1),), SENT, device="cuda")
    _lib.check(lib.wmf_row_transform_chained(_ptr(gd), m, f, ld, bias, _ptr(Nd), int(rolled), _ptr(body),
                                             _ptr(pairs) if bias else None, _stream()))
    b, p = body.cpu().numpy(), pairs.cpu().numpy()
    assert np.all(b[m * ldv:] == SENT) and np.all(p[m * (2 if split else 1):] == SENT), "written behind row m"
    b = b[: m * ldv].reshape(m, ldv)
    if split:
        p = p[: 2 * m].reshape(m, 2)
        return np.concatenate([b, p[:, :1]], axis=1), p[:, 1].copy(), b, p
    assert not b[:, f:].any(), "padding columns are not zero"
    return b[:, :f].copy(), (p[:m].copy() if bias else None), b, p


def _dense_n(f1, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((f1, f1)) * 2.0 ** rng.integers(-6, 2, (1, f1))).astype(np.float32)


@pytest.mark.parametrize("shape", ["anti", "dense"])
@pytest.mark.parametrize("f,bias", PASS_WIDTHS)
def test_chained_pass_short_last_chunk(f, bias, shape):
    _lib, lib, _ptr, _stream = _api()
    ld, f1 = lib.wmf_ld_for(f), f + bias
    rolled_ok = bool(bias and lib.wmf_rolled_layout_supported(f, ld))
    assert rolled_ok == (f == 129 and bias == 1)
    N = _dense_n(f1, 17 * f + bias)
    if shape == "anti":
        N[_predicted_zero(f, bias, rolled_ok)] = 0                # as the reversed compose leaves it, in the kernel's positions
    worst = 0.0
    for m in M_EDGES:
        g = _g_rows(m, f, seed=5 * f + m)
        a = _aug(g, bias)
        ref, mag = a @ N.astype(np.float64), np.abs(a) @ np.abs(N).astype(np.float64)
        got, bvec, body, pairs = _chained(g, N, bias, 0, ld)
        live = mag[:, :f] > 0                                     # (anti: row 0's column can be an empty sum)
        assert not got[~live].any()
        ratio = np.abs(got - ref[:, :f])[live] / (mag[:, :f][live] * U)
        print(f"chained pass {shape} f={f} bias={bias} m={m}: {ratio.max():.2f} u (gate {2 * (f1 + 2)})")
        assert ratio.max() <= 2 * (f1 + 2), (f, bias, m, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
        if bias:
            rb = np.abs(bvec - ref[:, f]) / (mag[:, f] * U)
            assert rb.max() <= 2 * (f1 + 2), (f, bias, m, float(rb.max()))
            worst = max(worst, float(rb.max()))
        again = _chained(g, N, bias, 0, ld)
        assert np.array_equal(_bits(got), _bits(again[0])) and np.array_equal(_bits(pairs), _bits(again[3]))
        if rolled_ok:
            got3, b3, body3, pairs3 = _chained(g, N, bias, 1, ld)
            stuffed = (np.arange(f - 1) % 8) < 2
            assert np.array_equal(_bits(body3[:, ~stuffed]), _bits(body[:, ~stuffed]))
            assert np.array_equal(_bits(body3[:, stuffed]) & ~np.uint32(1), _bits(body[:, stuffed]) & ~np.uint32(1)), \
                "more than the last mantissa bit moved"
            assert np.array_equal(_bits(pairs3), _bits(pairs))
            lsb = (_bits(body3[:, stuffed]) & np.uint32(1)).astype(np.uint64)
            rebuilt = (lsb << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
            assert np.array_equal(rebuilt, _bits(pairs3[:, 1])), "the stuffed bits are not the bias of the pairs"
            again3 = _chained(g, N, bias, 1, ld)
            assert np.array_equal(_bits(body3), _bits(again3[2]))
    record_error(f"reversed_pass[{shape},f={f},bias={bias}]", worst_u=worst, gate_u=2 * (f1 + 2))


# ------------------------------------------------------------------------------------------------------- 3. the engine
SLAB = 1 << 18


def _sample_rows(deg, n_random, n_extreme, rng):
    order = np.argsort(deg, kind="stable")
    pick = np.concatenate([order[-n_extreme:], order[:n_extreme], rng.choice(deg.size, min(n_random, deg.size), replace=False)])
    return np.unique(pick)


def _gramian64(Y_dev, f, lam, bias):
    y = Y_dev[:, :f].double()
    if bias:
        y[:, 0] = 1.0
    return (y.T @ y).cpu().numpy() + lam * np.eye(f)


def _gathered(csr, Y_dev, f, bias, lo, hi):
    idx = csr.indices[lo:hi].long()
    w = csr.values[lo:hi].double().cpu().numpy()
    Ug = Y_dev[idx][:, :f].double().cpu().numpy()
    if bias:
        w = w - Ug[:, 0]
        Ug[:, 0] = 1.0
    return Ug, w


def _check_side(eng, side, rng, n_random=400, n_extreme=50):
    """Worst relative row error of ``side`` (just solved) against oracle.solve_row on the fixed side's device factors
    (tests/test_gpu_scale.py, _check_side)."""
    fixed = "items" if side == "users" else "users"
    f, bias = eng.f, eng.bias
    csr = eng.csr[side]
    indptr = csr.indptr.cpu().numpy()
    deg = np.diff(indptr)[: eng.n[side]]
    rows = _sample_rows(deg, n_random, n_extreme, rng)
    Y_dev = eng.X[fixed]
    G = _gramian64(Y_dev[: eng.n[fixed]], f, eng.gamma, bias)
    got = eng.factors[side][torch.from_numpy(rows).to(eng.device)][:, :f].double().cpu().numpy()
    worst = 0.0
    for j, u in enumerate(rows):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi == lo:
            assert not got[j].any(), f"{side} row {u} has no entries and is not zero"
            continue
        assert hi - lo <= SLAB
        Ug, w = _gathered(csr, Y_dev, f, bias, lo, hi)
        want = orc.solve_row(G, Ug, np.arange(hi - lo), w)
        e, n_ = np.linalg.norm(got[j] - want), np.linalg.norm(want)
        assert np.isfinite(e), (side, int(u), hi - lo)
        worst = max(worst, e / n_)
    return worst


def _engine(bias, chained):
    from recmodel_amd import WMF, synth
    from recmodel_amd.engine import AlsEngine
    n_users, n_items, k = 3000, 400, 128
    ip, idx, val = synth.make_counts(n_users, n_items, 40, 1995, device="cuda")
    eng = AlsEngine(n_users, n_items, k, bias, 0.1, chained=chained)
    eng.set_interactions(ip, idx, 10 * torch.log(1 + val))
    eng.set_factors("items", WMF(num_items=n_items, num_users=1, dim=k, gamma=0.1, weighted=True, bias=bias).items)
    return eng


def _factors_from_g(eng, side):
    """g . U in float64 and its magnitude sum |g| |U|, g's positions put back in feature order."""
    f = eng.f
    n = eng.n[side]
    g = eng.g[side][:n, :f].double().cpu().numpy()
    Uw = eng.U[side][:, :f].double().cpu().numpy()
    if eng.rolled:
        g = g[:, (np.arange(f) - 1) % f]                          # position p holds feature p + 1 (f - 1: feature 0)
    return g @ Uw, np.abs(g) @ np.abs(Uw)


@pytest.mark.parametrize("bias", [True, False])
def test_engine_reversed_against_eager_and_oracle(bias):
    worst = {}
    for chained in (True, False):
        eng = _engine(bias, chained)
        assert eng.chained == chained and eng.rolled == bias
        f, f1 = eng.f, eng.f + int(bias)
        w = 0.0
        for it in range(3):
            for side in ("users", "items"):
                eng.half_step(side)
                eng.check_numerics()
                fixed = "users" if side == "items" else "items"
                if chained and (it, side) != (0, "users"):
                    # this half step whitened `fixed` straight from its g: N_ext is anti-triangular on either side ...
                    N = eng.N_ext[:, :f1].cpu().numpy()
                    assert not N[_predicted_zero(f, int(bias), eng.rolled)].any(), (it, side)
                    # ... and the un-whitening of the users' g is the anti-triangular L^-1 P^T, of the items' g the plain L^-1
                    Uw = eng.U[side][:, :f].cpu().numpy()
                    if fixed == "users":
                        i, j = np.indices((f, f))
                        assert not Uw[(i + j < f) & (j >= 1) if bias else (i + j < f - 1)].any() and np.triu(Uw, 1).any()
                    else:
                        assert not np.triu(Uw, 1).any()
                if chained and it == 1:
                    # the factors read mid-loop: g . U bit for bit (the un-whitening pass on the same operands), and within the
                    # row transform's per-element bound of float64
                    assert eng._owed[side]
                    want = torch.zeros_like(eng.g[side])
                    eng.K.row_transform(eng.g[side], eng.n_local[side], eng.f, eng.ld, eng.U[side], eng.unwhite_mode, want, None)
                    got = eng.factors[side]
                    assert not eng._owed[side] and torch.equal(got, want)
                    ref, mag = _factors_from_g(eng, side)
                    x = got[: eng.n[side], :f].double().cpu().numpy()
                    ok = mag > 0
                    ratio = np.abs(x - ref)[ok] / (mag[ok] * U)
                    assert ratio.max() <= 2 * (f + 2), (side, float(ratio.max()))
                if it == 2:
                    assert not chained or eng.g_valid[fixed]
                    w = max(w, _check_side(eng, side, np.random.default_rng(7)))
        worst[chained] = w
    record_error(f"reversed_engine[bias={bias}]", reversed_worst_row=worst[True], eager_worst_row=worst[False])
    print(f"engine bias={bias}: worst row reversed {worst[True]:.3e} eager {worst[False]:.3e}")
    assert worst[True] <= 2 * worst[False], worst
