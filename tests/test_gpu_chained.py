"""The chained whitening of a solved side (include/wmf_hip.h, "CHAINED WHITENING"): the three entry points
per element through the C ABI, and the engine that uses them.

With a = [g, 1] (bias) or a = g, and N_ext = [T . W_white | U[:, 0]]:
    wmf_gram_whitened          G_aug = a^T a
    wmf_compose_whitening      G~ = T^T G_aug T, its factorisation, N_ext
    wmf_row_transform_chained  a . N_ext in the layout wmf_row_transform(set_col0_one = bias / 3) writes
Every building-block case compares the device with NumPy float64 on the same float32 operands, with the per-element bounds
tests/test_gpu_dense.py applies to wmf_gram and wmf_row_transform: 2 (n + 2) u sum |x| |y| for a sum of n products in float32
(n u for the sum in any order, one u for the dropped products of the bf16 split, one for the final rounding, doubled for an
accumulator that truncates) -- n = m rows for the Gramian, n = f + bias terms for the row transform -- and the factorisation
gate of that file, u |L^-1| + 8 f cond2(A) 2^-53 max |L^-1|.  g's padding columns hold NaN throughout: they are not data.

The engine part runs three ALS iterations with and without the chained path from the same start and compares both with the
float64 oracle on the same rows: the chained run's worst row may be at most twice the eager run's (the two paths round
differently, neither is favoured)."""
import numpy as np
import pytest
import torch

from conftest import record_error

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_F = 8                                                           # tests/test_gpu_dense.py, the factorisation gate
SENT = 3.0
# (f, bias) the ABI supports among f in {97, 113, 128, 129, 144} x {0, 1}: not 128 and 144 with biases (ld = f there: no position
# for the one; 145 columns)
CASES = [(f, b) for f in (97, 113, 128, 129, 144) for b in (0, 1) if f + b <= min(144, (f + 3) & ~3)]
assert len(CASES) == 8
# 161: two waves of the Gramian, the second ends in a ragged chunk; 1, 15, 17, 31: a wave whose only chunk is ragged
M_EDGES = (1, 15, 16, 17, 31, 32, 33, 127, 129, 161)


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
    """[m, f] graded columns (the column norms of trained factors), drawn once and sliced."""
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


def test_supported_widths():
    _lib, lib, _ptr, _stream = _api()
    for f in (96, 97, 113, 128, 129, 143, 144, 145):
        ld = lib.wmf_ld_for(f)
        for bias in (0, 1):
            want = 97 <= f <= 144 and f + bias <= 144 and ld >= f + bias
            assert bool(lib.wmf_chained_supported(f, ld, bias)) == want, (f, ld, bias)
    assert not lib.wmf_chained_supported(143, 143, 0)            # (ld not a multiple of four)


# ------------------------------------------------------------------------------------------------------- 1. Gramian of g
@pytest.mark.parametrize("f,bias", CASES)
def test_gram_whitened_per_element(f, bias):
    _lib, lib, _ptr, _stream = _api()
    ld, f1 = lib.wmf_ld_for(f), f + bias
    ws = _ws(lib, f)
    worst = 0.0
    for m in M_EDGES:
        g = _g_rows(m, f, seed=3 * f + m)
        gd = _dev(_padded_nan(g, ld))
        out = []
        for _ in range(2):
            G = torch.full((f1 * f1,), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(lib.wmf_gram_whitened(_ptr(gd), m, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
            out.append(G.cpu().numpy().reshape(f1, f1))
        a = _aug(g, bias)
        ref, mag = a.T @ a, np.abs(a).T @ np.abs(a)
        ratio = np.abs(out[0] - ref) / (mag * U)
        worst = max(worst, float(ratio.max()))
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"gram_whitened f={f} bias={bias} m={m}: {ratio.max():.2f} u (gate {2 * (m + 2)})")
        assert ratio.max() <= 2 * (m + 2), (f, bias, m, k, float(ratio.max()), out[0][k], ref[k])
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[0].T)
        if bias:
            assert out[0][f, f] == m                              # the sum of m ones
    record_error(f"chained_gram[f={f},bias={bias}]", worst_u=worst)
    G = torch.full((f1 * f1,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.wmf_gram_whitened(_ptr(gd), 0, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
    assert not G.cpu().numpy().any()                              # no rows: a zero matrix


# ------------------------------------------------------------------------------------------------------- 2. the chained pass
def _chained(g, N, bias, rolled, ld):
    """wmf_row_transform_chained on g [m, f], N [f1, f1] (host).  Returns (the logical [m, f] whitened rows in the positions
    the call wrote them, the bias per row or None, body, pairs)."""
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


@pytest.mark.parametrize("f,bias", CASES)
def test_chained_pass_per_element(f, bias):
    _lib, lib, _ptr, _stream = _api()
    ld, f1 = lib.wmf_ld_for(f), f + bias
    N = _dense_n(f1, 17 * f + bias)
    rolled_ok = bool(bias and lib.wmf_rolled_layout_supported(f, ld))
    assert rolled_ok == (f == 129 and bias == 1)
    worst = 0.0
    for m in M_EDGES:
        g = _g_rows(m, f, seed=5 * f + m)
        a = _aug(g, bias)
        ref, mag = a @ N.astype(np.float64), np.abs(a) @ np.abs(N).astype(np.float64)
        got, bvec, body, pairs = _chained(g, N, bias, 0, ld)
        ratio = np.abs(got - ref[:, :f]) / (mag[:, :f] * U)
        assert ratio.max() <= 2 * (f1 + 2), (f, bias, m, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
        if bias:
            rb = np.abs(bvec - ref[:, f]) / (mag[:, f] * U)
            assert rb.max() <= 2 * (f1 + 2), (f, bias, m, float(rb.max()))
            worst = max(worst, float(rb.max()))
        again = _chained(g, N, bias, 0, ld)
        assert np.array_equal(_bits(got), _bits(again[0]))
        if rolled_ok:
            # the rolled call: the same sums (N_ext arrives in the kernel's coordinates either way); the 32 bits of the row's
            # bias replace the last mantissa bit of body positions 8 j, 8 j + 1 and nothing else moves
            got3, b3, body3, pairs3 = _chained(g, N, bias, 1, ld)
            stuffed = (np.arange(f - 1) % 8) < 2
            assert np.array_equal(_bits(body3[:, ~stuffed]), _bits(body[:, ~stuffed]))
            assert np.array_equal(_bits(body3[:, stuffed]) & ~np.uint32(1), _bits(body[:, stuffed]) & ~np.uint32(1)), \
                "more than the last mantissa bit moved"
            assert np.array_equal(_bits(pairs3), _bits(pairs))
            lsb = (_bits(body3[:, stuffed]) & np.uint32(1)).astype(np.uint64)        # bit 2 j + b of the bias, in that order
            rebuilt = (lsb << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
            assert np.array_equal(rebuilt, _bits(pairs3[:, 1])), "the stuffed bits are not the bias of the pairs"
    print(f"chained pass f={f} bias={bias}: worst {worst:.2f} u (gate {2 * (f1 + 2)})")
    record_error(f"chained_pass[f={f},bias={bias}]", worst_u=worst, gate_u=2 * (f1 + 2))


# ------------------------------------------------------------------------------------------------------- 3. compose
def _t_matrix(Uw, f, bias, rolled):
    """T [(f + bias), f] in float64, rows in g's positions."""
    src = (np.arange(f) + 1) % f if rolled else np.arange(f)
    T = Uw[src].astype(np.float64)
    if bias:
        T[:, 0] = 0
        T = np.concatenate([T, np.eye(1, f)], axis=0)
    return T


def _compose(Gaug, Uw, f, ld, bias, rolled, lam):
    _lib, lib, _ptr, _stream = _api()
    f1 = f + bias
    Ud = torch.zeros(f, ld, device="cuda")
    Ud[:, :f] = _dev(Uw)
    Ww, Wu, N = (torch.full((r, ld), 7.0, device="cuda") for r in (f, f, f1))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_compose_whitening(_ptr(_dev(Gaug.reshape(-1))), _ptr(Ud), f, ld, bias, int(rolled), lam, _ptr(Ww), _ptr(Wu),
                                         _ptr(N), _ptr(info), _ptr(_ws(lib, f)), _stream()))
    return Ww.cpu().numpy(), Wu.cpu().numpy(), N.cpu().numpy(), int(info[0])


@pytest.mark.parametrize("f,bias,rolled", [(f, b, 0) for f, b in CASES] + [(129, 1, 1)])
def test_compose_whitening(f, bias, rolled):
    _lib, lib, _ptr, _stream = _api()
    ld, f1, lam = lib.wmf_ld_for(f), f + bias, 0.1
    rng = np.random.default_rng(9000 + f + bias)
    # U: the un-whitening of a Gaussian Gramian (lower triangular, as the engine's); G_aug of 150 graded rows
    Y = rng.standard_normal((600, f))
    Uw = np.linalg.inv(np.linalg.cholesky(Y.T @ Y + lam * np.eye(f))).astype(np.float32)
    a = _aug(_g_rows(150, f, seed=f) * np.float32(8.0), bias)
    Gaug = a.T @ a
    Ww, Wu, N, info = _compose(Gaug, Uw, f, ld, bias, rolled, lam)
    assert info == 0
    T = _t_matrix(Uw, f, bias, rolled)
    A = T.T @ Gaug @ T + lam * np.eye(f)
    Linv, cond = np.linalg.inv(np.linalg.cholesky(A)), np.linalg.cond(A)
    bound = U * np.abs(Linv) + C_F * f * cond * 2.0 ** -53 * np.abs(Linv).max()
    err = np.abs(Wu[:, :f].astype(np.float64) - Linv)
    k = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (f, bias, k, err[k], bound[k], cond)
    assert np.array_equal(_bits(Ww[:, :f]), _bits(Wu[:, :f].T))
    assert not Wu[:, f:].any() and not Ww[:, f:].any()
    # ... and wmf_factorize on NumPy's T^T G_aug T gives the same matrices within the same gate
    Gd, Ww2, Wu2 = _dev((T.T @ Gaug @ T).reshape(-1)), torch.zeros(f, ld, device="cuda"), torch.zeros(f, ld, device="cuda")
    info2 = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.wmf_factorize(_ptr(Gd), f, ld, lam, _ptr(Ww2), _ptr(Wu2), _ptr(info2), _ptr(ws), _stream()))
    assert np.all(np.abs(Wu[:, :f].astype(np.float64) - Wu2.cpu().numpy()[:, :f]) <= 2 * bound)
    # N_ext = [T . W_white | U[:, 0]] from the float32 W_white the call returned, columns in the whitened side's positions
    col = (np.arange(f) + 1) % f if rolled else np.arange(f)
    W64 = Ww[:, :f].astype(np.float64)[:, col]
    ref, mag = T @ W64, np.abs(T) @ np.abs(W64)
    assert np.all(np.abs(N[:, :f] - ref) <= U * np.abs(ref) + f * 2.0 ** -52 * mag)
    if bias:
        src = (np.arange(f) + 1) % f if rolled else np.arange(f)
        assert np.array_equal(_bits(N[:f, f]), _bits(Uw[src, 0])) and N[f, f] == 0
    assert not N[:, f1:].any()
    # a Gramian that is not positive definite: info names the minor, the outputs are zero matrices
    Ww, Wu, N, info = _compose(-Gaug - np.eye(f1), Uw, f, ld, bias, rolled, lam)
    assert info >= 1 and not Ww.any() and not Wu.any() and not N[:, :f].any()


# ------------------------------------------------------------------------------------------------------- 4. the engine
def _engine(bias, chained, kernels=None):
    from recmodel_amd import WMF, synth
    from recmodel_amd.engine import AlsEngine
    n_users, n_items, k = 3000, 400, 128
    ip, idx, val = synth.make_counts(n_users, n_items, 40, 1995, device="cuda")
    eng = AlsEngine(n_users, n_items, k, bias, 0.1, chained=chained)
    eng.set_interactions(ip, idx, 10 * torch.log(1 + val))
    eng.set_factors("items", WMF(num_items=n_items, num_users=1, dim=k, gamma=0.1, weighted=True, bias=bias).items)
    return eng


@pytest.mark.parametrize("bias", [True, False])
def test_engine_chained_against_eager_and_oracle(bias):
    from test_gpu_scale import _check_side
    worst = {}
    for chained in (True, False):
        eng = _engine(bias, chained)
        assert eng.chained == chained and eng.rolled == bias
        w = 0.0
        for it in range(3):
            for side in ("users", "items"):
                eng.half_step(side)
                eng.check_numerics()
                if it == 2:                                       # the third iteration: both sides came out of the chained route
                    assert not chained or eng.g_valid["users" if side == "items" else "items"]
                    r = _check_side(eng, side, np.random.default_rng(7), (np.inf, np.inf), n_random=400, n_extreme=50)
                    w = max(w, r[0])
        worst[chained] = w
    record_error(f"chained_engine[bias={bias}]", chained_worst_row=worst[True], eager_worst_row=worst[False])
    print(f"engine bias={bias}: worst row chained {worst[True]:.3e} eager {worst[False]:.3e}")
    assert worst[True] <= 2 * worst[False], worst


@pytest.mark.parametrize("bias", [True, False])
def test_engine_materialises_on_read(bias):
    eng = _engine(bias, True)
    K = eng.K

    def unwhitened(side):
        out = torch.zeros_like(eng.g[side])
        K.row_transform(eng.g[side], eng.n_local[side], eng.f, eng.ld, eng.U[side], eng.unwhite_mode, out, None)
        return out

    eng.half_step("users")                                        # items were set: today's path, un-whitening included
    assert eng.g_valid["users"] and not eng.g_valid["items"] and not eng._owed["users"]
    assert torch.equal(eng.factors["users"], unwhitened("users"))
    eng.half_step("items")                                        # chained: from g["users"]; the items' factors are owed
    assert eng.g_valid["items"] and eng._owed["items"]
    want = unwhitened("items")
    assert torch.equal(eng.factors["items"], want) and not eng._owed["items"]
    eng.half_step("users")
    assert eng._owed["users"]
    for read in ("factors", "X", "get_factors"):
        eng._owed["users"] = True                                 # (owed again: every reader writes the same bits)
        dict.__getitem__(eng.factors, "users").fill_(5.0)
        got = {"factors": lambda: eng.factors["users"], "X": lambda: eng.X["users"],
               "get_factors": lambda: torch.from_numpy(eng.get_factors("users")).cuda()}[read]()
        assert torch.equal(got[:, : eng.f], unwhitened("users")[: eng.n["users"], : eng.f]), read
    # the same half step twice, with and without a read of the fixed side in between: the same bits
    eng.half_step("items")
    first = eng.g["items"].clone()
    eng.half_step("items")
    assert torch.equal(first, eng.g["items"])
    _ = eng.factors["users"], eng.X["users"]
    eng.half_step("items")
    assert torch.equal(first, eng.g["items"])
    # set_factors after a solve: the next half step whitens the factors that were set
    full = eng.get_factors("users")
    eng.set_factors("users", full * np.float32(0.5))
    assert not eng.g_valid["users"] and not eng._owed["users"]
    eng.half_step("items")
    eager = _engine(bias, False)
    eager.set_factors("users", full * np.float32(0.5))
    eager.half_step("items")
    assert torch.equal(eng.factors["items"], eager.factors["items"])


def test_fake_kernels_engine_takes_the_eager_path():
    from fake_kernels import NumpyKernels
    from recmodel_amd import synth
    from recmodel_amd.engine import AlsEngine
    ip, idx, val = synth.make_counts(60, 40, 6, 3)
    eng = AlsEngine(60, 40, 128, True, 0.1, device="cpu", kernels=NumpyKernels())
    assert not eng.chained
    eng.set_interactions(ip, idx, val)
    eng.set_factors("items", np.random.default_rng(1).standard_normal((40, eng.f)).astype(np.float32) * 0.1)
    eng.half_step("users")
    eng.half_step("items")
    assert not eng._owed["users"] and np.isfinite(eng.get_factors("users")).all()
