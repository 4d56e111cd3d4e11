"""wmf_posterior_draw_rows, wmf_posterior_score_rows and wmf_posterior_noise through the C ABI (tests/posterior_ref.py): the hash bit
for bit and the variates against float64; sigma = 0 against wmf_foldin_rows bit for bit on the same buffers; draws and scores
within the fold-in's two-term gate (4 x the error of the float32 restatement + 8 ulps of the float64 definition) given the
device's own variates; the invariances (draw prefixes, target columns, a row alone or moved, two runs); the exactly orthogonal
catalogue against fractions.Fraction; the covariance of 4096 draws; the properties of a variance; the means against
wmf_explain_rows's totals; the failure report and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref
import foldin_ref
import posterior_ref as ref
from conftest import record_error

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64
SIGMA = 0.5


def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()             # (a copy: the shared cases are read-only)


def _upload(c):
    """The inputs of case c on the device (one spare element each: never empty)."""
    return dict(Y=_dev(c["Y"]), W=_dev(c["W32"]), indices=_dev(np.append(c["indices"], 0), np.int32),
                values=_dev(np.append(c["values"], 0), np.float32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _guarded(n_floats):
    return torch.full((n_floats + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def _inside(t, shape):
    h = t.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "output guards"
    return h[GUARD:-GUARD].reshape(shape)


def _row_args(c, d, first, count, _ptr):
    ip = _dev(c["indptr"][first:first + count + 1], np.int64)
    return ip, dict(Y=_ptr(d["Y"]), m=c["m"], f=c["f"], ld=c["ld"], bias=c["bias"], W=_ptr(d["W"]), indptr=_ptr(ip), indices=_ptr(d["indices"]),
                    values=_ptr(d["values"]), n=count)


ROW_KEYS = ("Y", "m", "f", "ld", "bias", "W", "indptr", "indices", "values", "n")


def _foldin(c, bufs):
    _lib, lib, _ptr, _stream = _api()
    n = len(c["indptr"]) - 1
    ip, a = _row_args(c, bufs, 0, n, _ptr)
    X = torch.full((n, c["ld"]), SENTINEL, dtype=torch.float32, device="cuda")
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = int(lib.wmf_foldin_workspace_bytes(n, c["f"]))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wmf_foldin_rows(*[a[k] for k in ROW_KEYS], _ptr(X), _ptr(fail), _ptr(ws), need, _stream()))
    torch.cuda.synchronize()
    return X.cpu().numpy(), int(fail[0])


def _draw(c, n_draws, sigma, seed=7, streams=None, first=0, count=None, expect=0, bufs=None, args=None):
    """n_draws draws of rows [first, first + count) of case c through an indptr window.  Returns (X [count, n_draws, ld], fail count);
    the guards around the output, the failure counter and the workspace are checked here.  args: arguments of the call to replace."""
    _lib, lib, _ptr, _stream = _api()
    n_all = len(c["indptr"]) - 1
    count = n_all - first if count is None else count
    d = bufs or _upload(c)
    ip, a = _row_args(c, d, first, count, _ptr)
    st = None if streams is None else _dev(np.asarray(streams, dtype=np.uint64).view(np.int64))
    X = _guarded(count * n_draws * c["ld"])
    fail = torch.tensor([-7, 0, -7], dtype=torch.int32, device="cuda")
    need = int(lib.wmf_posterior_draw_workspace_bytes(count, c["f"], n_draws))
    ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    a.update(n_draws=n_draws, sigma=sigma, seed=seed, row_stream=_ptr(st), X=ctypes.c_void_p(X.data_ptr() + 4 * GUARD),
             fail=ctypes.c_void_p(fail.data_ptr() + 4), ws=_ptr(ws), ws_bytes=need)
    a.update(args or {})
    rc = lib.wmf_posterior_draw_rows(*[a[k] for k in ROW_KEYS + ("n_draws", "sigma", "seed", "row_stream", "X", "fail", "ws", "ws_bytes")],
                                     _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.wmf_last_error())
    fh = fail.cpu().numpy()
    assert fh[0] == -7 and fh[2] == -7, "fail_count guards"
    assert (ws.cpu().numpy() == 0x5A).all(), "the workspace is reserved, not written"
    return _inside(X, (count, n_draws, c["ld"])), int(fh[1])


def _score(c, targets, first=0, count=None, expect=0, bufs=None, want=(True, True), args=None):
    """mean and var of targets [count, T] for rows [first, first + count).  Returns (mean, var, fail count), None for an output not
    asked for."""
    _lib, lib, _ptr, _stream = _api()
    n_all = len(c["indptr"]) - 1
    count = n_all - first if count is None else count
    T = targets.shape[1]
    d = bufs or _upload(c)
    ip, a = _row_args(c, d, first, count, _ptr)
    tg = _dev(np.append(np.asarray(targets).reshape(-1), 0), np.int32)
    outs = [_guarded(count * T) if w else None for w in want]
    fail = torch.tensor([-7, 0, -7], dtype=torch.int32, device="cuda")
    need = int(lib.wmf_posterior_score_workspace_bytes(count, c["f"], T))
    ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    a.update(targets=_ptr(tg), n_targets=T, fail=ctypes.c_void_p(fail.data_ptr() + 4), ws=_ptr(ws), ws_bytes=need,
             mean=ctypes.c_void_p(outs[0].data_ptr() + 4 * GUARD) if want[0] else None,
             var=ctypes.c_void_p(outs[1].data_ptr() + 4 * GUARD) if want[1] else None)
    a.update(args or {})
    rc = lib.wmf_posterior_score_rows(*[a[k] for k in ROW_KEYS + ("targets", "n_targets", "mean", "var", "fail", "ws", "ws_bytes")], _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.wmf_last_error())
    fh = fail.cpu().numpy()
    assert fh[0] == -7 and fh[2] == -7, "fail_count guards"
    assert (ws.cpu().numpy() == 0x5A).all(), "the workspace is reserved, not written"
    return tuple(None if o is None else _inside(o, (count, T)) for o in outs) + (int(fh[1]),)


def _noise(seed, streams, draws, comps, want=(True, True)):
    _lib, lib, _ptr, _stream = _api()
    n = len(draws)
    st = None if streams is None else _dev(np.asarray(streams, dtype=np.uint64).view(np.int64))
    xi = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda") if want[0] else None
    k = torch.full((n, 2), -1, dtype=torch.int32, device="cuda") if want[1] else None
    draws_d, comps_d = _dev(draws, np.int32), _dev(comps, np.int32)                  # (held until the synchronize)
    _lib.check(lib.wmf_posterior_noise(seed, _ptr(st), _ptr(draws_d), _ptr(comps_d), n, _ptr(xi), _ptr(k), _stream()))
    torch.cuda.synchronize()
    return (None if xi is None else xi.cpu().numpy()), (None if k is None else k.cpu().numpy().view(np.uint32))


def _xi_of(seed, streams, n_draws, f):
    """float32 [len(streams), n_draws, f]: the device's own variates of those rows."""
    n = len(streams)
    s, d, a = np.meshgrid(np.asarray(streams, dtype=np.uint64), np.arange(n_draws), np.arange(f), indexing="ij")
    xi, _ = _noise(seed, s.ravel(), d.ravel(), a.ravel(), want=(True, False))
    return xi.reshape(n, n_draws, f)


# ---------------------------------------------------------------------------------------------------- 1. the noise
def test_noise_bits_and_values():
    """k1, k2 of 2^20 triples bit for bit -- draw and component at 0 and at their maxima (the kernel's: 4095 and 259; the entry's:
    2^31 - 1), seed and stream 2^64 - 1 -- and xi against float64.  The gate on xi is twice the worst error measured on an MI355X,
    1.84 units of 2^-23 max(1, |xi|) (profiles/r26_posterior.json); every exact test below uses the read-back xi, so this gate guards
    nothing else."""
    rng = np.random.default_rng(1)
    N = 1 << 20
    streams = rng.integers(0, 2 ** 63, N).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, N).astype(np.uint64)
    draws, comps = rng.integers(0, ref.MAX_DRAWS, N), rng.integers(0, ref.MAX_F, N)
    streams[:4] = [0, 1, 2 ** 64 - 1, 2 ** 63]
    draws[:8] = [0, ref.MAX_DRAWS - 1, 0, ref.MAX_DRAWS - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 1]
    comps[:8] = [0, 0, ref.MAX_F - 1, ref.MAX_F - 1, 2 ** 31 - 1, 0, 2 ** 31 - 1, 1]
    worst = 0.0
    for seed in (2 ** 64 - 1, 0, 12345):
        xi, k = _noise(seed, streams, draws, comps)
        k1, k2 = ref.normal_k(seed, streams, draws, comps)
        assert np.array_equal(k[:, 0], k1) and np.array_equal(k[:, 1], k2)
        for i in range(8):
            assert (int(k[i, 0]), int(k[i, 1])) == ref.normal_k_int(seed, int(streams[i]), int(draws[i]), int(comps[i]))
        want = ref.xi64(k1, k2)
        assert np.abs(xi).max() <= ref.XI_BOUND
        worst = max(worst, float((np.abs(xi - want) / (2.0 ** -23 * np.maximum(1.0, np.abs(want)))).max()))
    print(f"xi against float64: worst error {worst:.3f} x 2^-23 max(1, |xi|)")
    record_error("posterior", xi_error_units=worst)
    assert worst <= 2 * 1.84
    # row_stream == NULL: stream = the position; one output at a time: the same bits
    xi0, k0 = _noise(5, None, draws[:1000], comps[:1000])
    xi1, k1_ = _noise(5, np.arange(1000), draws[:1000], comps[:1000])
    assert np.array_equal(_bits(xi0), _bits(xi1)) and np.array_equal(k0, k1_)
    assert np.array_equal(_bits(_noise(5, None, draws[:1000], comps[:1000], want=(True, False))[0]), _bits(xi0))
    assert np.array_equal(_noise(5, None, draws[:1000], comps[:1000], want=(False, True))[1], k0)


# ---------------------------------------------------------------------------------------------------- 2. sigma = 0
@pytest.mark.parametrize("name", ref.identity_case_names())
def test_sigma_zero_is_the_fold_in_bit_for_bit(name):
    """Widths 1, 5, 30, 31, 32, 64, 129, 260 with and without biases at both leading dimensions, degrees 0 .. 3, 7 .. 9, f - 1 ..
    f + 1 and 33 with empty rows first, in the middle and last, the 9000-entry row, 1030 rows: one draw (the whole workgroup on the
    substitution) and three (a 16-lane group per draw) are both the fold-in, on the same device buffers, for any seed."""
    c = foldin_ref.case(name)
    bufs = _upload(c)
    want, want_fail = _foldin(c, bufs)
    assert want_fail == 0
    for n_draws, seed in ((1, 0), (3, 99)):
        X, fail = _draw(c, n_draws, 0.0, seed=seed, bufs=bufs)
        assert fail == want_fail and not (X == SENTINEL).any()
        for s in range(n_draws):
            assert np.array_equal(_bits(X[:, s]), _bits(want)), (name, n_draws, s)


@pytest.mark.parametrize("name", ["width_f64_b1_x4", "width_f5_b0_x4"])
def test_indptr_windows(name):
    c = foldin_ref.case(name)
    for sigma in (0.0, SIGMA):
        full, _ = _draw(c, 2, sigma, streams=np.arange(13))
        for first, count in ((2, None), (5, 3), (9, 1), (4, 1)):
            n = (13 - first) if count is None else count
            X, fail = _draw(c, 2, sigma, first=first, count=count, streams=np.arange(first, first + n))
            assert fail == 0 and np.array_equal(_bits(X), _bits(full[first:first + n]))
    tg = ref.targets_for(c, 5)
    mean, var, _ = _score(c, tg)
    for first, count in ((2, 11), (5, 3), (9, 1)):
        m, v, fail = _score(c, tg[first:first + count], first=first, count=count)
        assert fail == 0 and np.array_equal(_bits(m), _bits(mean[first:first + count])) and np.array_equal(_bits(v), _bits(var[first:first + count]))


# ---------------------------------------------------------------------------------------------------- 3. draws, sigma > 0
@pytest.mark.parametrize("name", ref.gated_case_names())
def test_draws_within_the_gate(name):
    """Three draws a row (a group per draw) and one (the whole workgroup; the bits of draw 0) against the float64 definition under
    the device's own variates: every live row and draw within 4 x the error of the float32 restatement on it + 8 ulps.  Empty rows
    are draws from the prior and are held to the same gate."""
    c = foldin_ref.case(name)
    n, f, D = len(c["indptr"]) - 1, c["f"], 3
    Yf = c["Y"][:, :f]
    bufs = _upload(c)
    X, fail = _draw(c, D, SIGMA, seed=3, bufs=bufs)
    assert fail == 0 and not (X == SENTINEL).any() and (_bits(X[:, :, f:]) == 0).all() and np.isfinite(X).all()
    one, _ = _draw(c, 1, SIGMA, seed=3, bufs=bufs)
    assert np.array_equal(_bits(one[:, 0]), _bits(X[:, 0]))
    xi = _xi_of(3, np.arange(n), D, f)
    want = ref.draws64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], xi.astype(np.float64), SIGMA)
    r32 = ref.restated_draws32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], xi, SIGMA)
    restated = ref.draw_errors(r32, want)
    err, gate = ref.draw_errors(X[:, :, :f], want), ref.gate_of(restated)
    assert (err <= gate).all(), (name, [(int(u), int(s), float(err[u, s]), float(gate[u, s])) for u, s in zip(*np.nonzero(err > gate))][:5])
    multiple = float(((err - ref.GATE_FLOOR) / np.maximum(restated, ref.TINY)).max())
    print(f"{name}: draw error {err.max():.3e}, restated {restated.max():.3e}, (error - floor) / restated at most {multiple:.3f} (gate: 4)")
    record_error("posterior", **{name + "_draw": err.max(), name + "_draw_restated": restated.max(), name + "_draw_multiple": multiple,
                                 name + "_draw_bits_equal_restated": float((_bits(X[:, :, :f]) == _bits(r32)).mean())})


def test_draw_s_does_not_depend_on_the_call():
    """n_draws 1, 2, 15, 16, 17 are prefixes of n_draws 100; a row alone, and rows moved to other positions with their row_stream
    entries, give the same bits; so do two runs."""
    c = foldin_ref.case("width_f129_b1_x0")
    bufs = _upload(c)
    streams = np.arange(13, dtype=np.uint64) * np.uint64(1000003) + np.uint64(2 ** 63)
    full, _ = _draw(c, 100, SIGMA, streams=streams, bufs=bufs)
    again, _ = _draw(c, 100, SIGMA, streams=streams, bufs=bufs)
    assert np.array_equal(_bits(full), _bits(again)) and np.isfinite(full).all()
    assert len({_bits(full[5, s, :8]).tobytes() for s in range(100)}) == 100         # (the draws differ)
    for n_draws in (1, 2, 15, 16, 17):
        X, _ = _draw(c, n_draws, SIGMA, streams=streams, bufs=bufs)
        assert np.array_equal(_bits(X), _bits(full[:, :n_draws])), n_draws
    alone, _ = _draw(c, 17, SIGMA, streams=streams[10:11], first=10, count=1, bufs=bufs)
    assert np.array_equal(_bits(alone[0]), _bits(full[10, :17]))
    ip, rows = c["indptr"], (10, 3, 0)                                               # (row 0 is empty: a draw from the prior)
    moved = dict(c)
    moved["indices"] = np.concatenate([c["indices"][ip[r]:ip[r + 1]] for r in rows])
    moved["values"] = np.concatenate([c["values"][ip[r]:ip[r + 1]] for r in rows])
    moved["indptr"] = np.concatenate([[0], np.cumsum([ip[r + 1] - ip[r] for r in rows])]).astype(np.int64)
    m, _ = _draw(moved, 17, SIGMA, streams=streams[list(rows)])
    for k, r in enumerate(rows):
        assert np.array_equal(_bits(m[k]), _bits(full[r, :17]))
    # row_stream == NULL is stream = the row's position, and another seed is another draw
    a, _ = _draw(c, 2, SIGMA, bufs=bufs)
    b, _ = _draw(c, 2, SIGMA, streams=np.arange(13), bufs=bufs)
    other, _ = _draw(c, 2, SIGMA, seed=8, bufs=bufs)
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(other))


def test_orthogonal_catalogue_draws_against_fractions():
    """Items are scaled unit vectors: the row system is diagonal and a draw's component is W_a b_a / L_aa^2 + W_a sigma xi / L_aa, in
    exact rational arithmetic (the square root to 160 bits) on the float32 inputs and the device's xi.  The device is held to 2 x the
    worst ulp error of the float32 restatement."""
    c, parts = ref.orthogonal_parts()
    n, f, D = len(c["indptr"]) - 1, c["f"], 17
    X, fail = _draw(c, D, SIGMA, seed=21)
    assert fail == 0
    xi = _xi_of(21, np.arange(n), D, f)
    r32 = ref.restated_draws32(c["Y"][:, :f], 0, c["W32"], c["indptr"], c["indices"], c["values"], xi, SIGMA)
    worst = restated = 0.0
    for u in range(n):
        for s in (0, 1, 16):
            for a in range(f):
                exact = ref.orthogonal_exact_draw(parts, u, a, SIGMA, xi[u, s, a])
                worst = max(worst, ref.ulp_error(X[u, s, a], exact))
                restated = max(restated, ref.ulp_error(r32[u, s, a], exact))
    print(f"orthogonal catalogue, draws: device {worst:.3f} ulp, restatement {restated:.3f} ulp")
    record_error("posterior", orthogonal_draw_ulp=worst, orthogonal_draw_ulp_restated=restated)
    assert worst <= 2.0 * restated


# ---------------------------------------------------------------------------------------------------- 4. draw statistics
@pytest.mark.parametrize("bias", [0, 1])
def test_the_covariance_of_4096_draws(bias):
    """f = 5, one history of 7 entries, 4096 draws under three seeds: N [tr(S C^-1) - log det(S C^-1) - f], S the sample covariance
    around the float64 fold-in and C = sigma^2 A_u^-1 in float64, is chi-square with 15 degrees of freedom for draws from N(x_u, C);
    the gate is its 99.9 % point, and the float64 reference's own draws lie under it (tests/test_posterior_cpu.py)."""
    c = ref.stat_case(bias)
    bufs = _upload(c)
    for seed in ref.STAT_SEEDS:
        X, fail = _draw(c, ref.MAX_DRAWS, ref.STAT_SIGMA, seed=seed, bufs=bufs)
        assert fail == 0
        stat = ref.covariance_statistic(X[0, :, :5], c["x"], c["cov"])
        print(f"bias {bias} seed {seed}: statistic {stat:.2f}, the reference's own {ref.reference_statistic(c, seed):.2f}, gate {ref.CHI2_15_999}")
        record_error("posterior", **{f"covariance_statistic_b{bias}_seed{seed}": stat})
        assert stat < ref.CHI2_15_999
        assert np.abs(X[0, :, :5].astype(np.float64).mean(axis=0) - c["x"]).max() <= 4.5 * np.sqrt(np.diag(c["cov"]).max() / ref.MAX_DRAWS)


# ---------------------------------------------------------------------------------------------------- 5. scores
def _check_scores(c, tg, mean, var, label):
    """Every element written, -1 slots exactly zero, var >= 0, and both outputs within their gates; returns the worst error / gate."""
    Yf = c["Y"][:, :c["f"]]
    assert not (mean == SENTINEL).any() and not (var == SENTINEL).any()
    assert (_bits(mean[tg < 0]) == 0).all() and (_bits(var[tg < 0]) == 0).all()
    assert np.isfinite(mean).all() and (var >= 0).all() and (var[tg >= 0] > 0).all()
    m64, v64, M = ref.scores64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], tg)
    m32, v32 = ref.restated_scores32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], tg)
    worst = {}
    for what, got, r32, want, scale in (("var", var, v32, v64, v64), ("mean", mean, m32, m64, M)):
        live = tg >= 0
        restated = np.where(live, ref.score_errors(r32, want, scale), 0.0)
        err, gate = np.where(live, ref.score_errors(got, want, scale), 0.0), ref.gate_of(restated)
        assert (err <= gate).all(), (label, what, [(int(u), int(t), float(err[u, t]), float(gate[u, t])) for u, t in zip(*np.nonzero(err > gate))][:5])
        worst[what] = (float(err.max()), float(restated.max()), float(((err - ref.GATE_FLOOR) / np.maximum(restated, ref.TINY)).max()))
    empty = np.diff(c["indptr"]) == 0
    Yt, beta = ref.tilde(Yf, c["bias"])
    for u in np.nonzero(empty)[0]:
        assert np.array_equal(mean[u][tg[u] >= 0], beta[tg[u][tg[u] >= 0]].astype(np.float32))      # an empty row: beta_i exactly
    print(f"{label}: var error {worst['var'][0]:.3e} (restated {worst['var'][1]:.3e}, multiple {worst['var'][2]:.3f}), "
          f"mean error {worst['mean'][0]:.3e} (restated {worst['mean'][1]:.3e}, multiple {worst['mean'][2]:.3f})")
    record_error("posterior", **{label + "_var": worst["var"][0], label + "_var_multiple": worst["var"][2], label + "_mean": worst["mean"][0],
                                 label + "_mean_multiple": worst["mean"][2]})


@pytest.mark.parametrize("name", ref.gated_case_names())
def test_scores_within_the_gate(name):
    """17 targets a row (two passes): items 0 and m - 1, an item of the row's own history, the same item twice (the same bits), -1
    slots (zeros), at every width and for the six weight families."""
    c = foldin_ref.case(name)
    tg = ref.targets_for(c, 17)
    mean, var, fail = _score(c, tg)
    assert fail == 0
    assert np.array_equal(_bits(mean[:, 0]), _bits(mean[:, -1])) and np.array_equal(_bits(var[:, 0]), _bits(var[:, -1]))
    _check_scores(c, tg, mean, var, name)


def test_target_counts_and_what_a_target_does_not_depend_on():
    """n_targets 1, 2, 15, 16, 17, 300 are column prefixes of n_targets 4096, bit for bit; a column alone, a row alone and a row moved
    give the same bits; so do two runs and a call with one output NULL.  All 4096 columns are gated."""
    c = foldin_ref.case("width_f64_b1_x0")
    bufs = _upload(c)
    tg = ref.targets_for(c, ref.MAX_TARGETS)
    mean, var, fail = _score(c, tg, bufs=bufs)
    assert fail == 0
    _check_scores(c, tg, mean, var, "targets_4096")
    again = _score(c, tg, bufs=bufs)
    assert np.array_equal(_bits(again[0]), _bits(mean)) and np.array_equal(_bits(again[1]), _bits(var))
    for T in (1, 2, 15, 16, 17, 300):
        m, v, _ = _score(c, tg[:, :T], bufs=bufs)
        assert np.array_equal(_bits(m), _bits(mean[:, :T])) and np.array_equal(_bits(v), _bits(var[:, :T])), T
    for t in (3, 16, 4095):
        m, v, _ = _score(c, tg[:, t:t + 1], bufs=bufs)
        assert np.array_equal(_bits(m[:, 0]), _bits(mean[:, t])) and np.array_equal(_bits(v[:, 0]), _bits(var[:, t]))
    m, v, _ = _score(c, tg[10:11, :300], first=10, count=1, bufs=bufs)
    assert np.array_equal(_bits(m[0]), _bits(mean[10, :300])) and np.array_equal(_bits(v[0]), _bits(var[10, :300]))
    ip, rows = c["indptr"], (10, 3, 0)
    moved = dict(c)
    moved["indices"] = np.concatenate([c["indices"][ip[r]:ip[r + 1]] for r in rows])
    moved["values"] = np.concatenate([c["values"][ip[r]:ip[r + 1]] for r in rows])
    moved["indptr"] = np.concatenate([[0], np.cumsum([ip[r + 1] - ip[r] for r in rows])]).astype(np.int64)
    m, v, _ = _score(moved, tg[list(rows), :300])
    assert np.array_equal(_bits(m), _bits(mean[list(rows), :300])) and np.array_equal(_bits(v), _bits(var[list(rows), :300]))
    only_mean = _score(c, tg[:, :17], bufs=bufs, want=(True, False))
    only_var = _score(c, tg[:, :17], bufs=bufs, want=(False, True))
    assert only_mean[1] is None and only_var[0] is None
    assert np.array_equal(_bits(only_mean[0]), _bits(mean[:, :17])) and np.array_equal(_bits(only_var[1]), _bits(var[:, :17]))


@pytest.mark.parametrize("name", ["gauss_f16_b0", "w1e3_f129_b1", "zeros_f260_b0", "dup_f65_b1", "eqbias_f16_b0"])
def test_a_history_only_narrows_the_prior(name):
    """Families whose effective weights are >= 0: var <= |q_i|^2, the prior variance, which is what the empty row of the case
    returns for the same item (all rows are given one target list); equal for the empty row itself, within the gate.  The slack of
    the comparison is the two gates, in float64 terms."""
    c = foldin_ref.case(name)
    f, n = c["f"], len(c["indptr"]) - 1
    Yf = c["Y"][:, :f]
    Yt, beta = ref.tilde(Yf, c["bias"])
    w = c["values"] - beta[c["indices"]]
    assert (w >= 0).all() and c["indptr"][1] == 0
    tg = np.tile(ref.targets_for(c, 40)[3], (n, 1))
    mean, var, fail = _score(c, tg)
    assert fail == 0 and (var >= 0).all()
    _, v64, _ = ref.scores64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], tg)
    _, v32 = ref.restated_scores32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], tg)
    gate = ref.gate_of(ref.score_errors(v32, v64, v64))
    live = tg[0] >= 0
    prior64 = ((Yt[tg[0][live]] @ ref.whitening(Yf, c["bias"], c["lam"])) ** 2).sum(axis=1)
    assert (np.abs(var[0, live] - prior64) <= gate[0, live] * prior64).all()
    for u in range(1, n):
        assert (var[u, live].astype(np.float64) <= var[0, live] * (1 + gate[u, live] + gate[0, live])).all(), (name, u)


def test_var_does_not_increase_when_a_positive_entry_is_appended():
    """Row k holds the first k entries of one history, k = 0 .. 12: each appended entry has a positive weight, so A_u grows in the
    Loewner order and every variance falls or stays; compared in float64 with the two gates as slack."""
    base = foldin_ref.case("width_f32_b1_x0")
    f = base["f"]
    lo = int(base["indptr"][9])
    hist, vals = base["indices"][lo:lo + 12], base["values"][lo:lo + 12]
    assert (vals - base["Y"][hist, 0] > 0).all()
    c = dict(base)
    c["indptr"] = np.concatenate([[0], np.cumsum(np.arange(13))]).astype(np.int64)
    c["indices"] = np.concatenate([hist[:k] for k in range(13)]).astype(np.int32)
    c["values"] = np.concatenate([vals[:k] for k in range(13)]).astype(np.float32)
    tg = np.tile(np.concatenate([hist, np.arange(0, 600, 23)]).astype(np.int32), (13, 1))
    mean, var, fail = _score(c, tg)
    assert fail == 0
    Yf = c["Y"][:, :f]
    _, v64, _ = ref.scores64(Yf, 1, c["lam"], c["indptr"], c["indices"], c["values"], tg)
    _, v32 = ref.restated_scores32(Yf, 1, c["W32"], c["indptr"], c["indices"], c["values"], tg)
    gate = ref.gate_of(ref.score_errors(v32, v64, v64))
    assert (np.diff(v64, axis=0) <= 0).all()
    for k in range(12):
        assert (var[k + 1].astype(np.float64) <= var[k] * (1 + gate[k] + gate[k + 1])).all(), k
    assert (v64[12, :12] < v64[0, :12] * (1 - 1e-3)).all() and (var[12, :12] < var[0, :12]).all()      # the history's own items: narrower


def test_orthogonal_catalogue_scores_against_fractions():
    """The exact rationals of tests/posterior_ref.py::orthogonal_parts: var = (s_i W_a)^2 / L_aa^2 and mean = s_i W_a b_a / L_aa^2; the
    mean of an item on an axis the history misses is exactly 0.  The device is held to 2 x the restatement's worst ulp error."""
    c, parts = ref.orthogonal_parts()
    n, m = len(c["indptr"]) - 1, c["m"]
    tg = np.tile(np.arange(m, dtype=np.int32), (n, 1))
    mean, var, fail = _score(c, tg)
    assert fail == 0
    m32, v32 = ref.restated_scores32(c["Y"][:, :c["f"]], 0, c["W32"], c["indptr"], c["indices"], c["values"], tg)
    worst, restated = [0.0, 0.0], [0.0, 0.0]
    for u in range(n):
        for i in range(m):
            em, ev = ref.orthogonal_exact_score(c, parts, u, i)
            worst[1], restated[1] = max(worst[1], ref.ulp_error(var[u, i], ev)), max(restated[1], ref.ulp_error(v32[u, i], ev))
            if em == 0:
                assert mean[u, i] == 0.0
            else:
                worst[0], restated[0] = max(worst[0], ref.ulp_error(mean[u, i], em)), max(restated[0], ref.ulp_error(m32[u, i], em))
    print(f"orthogonal catalogue, scores: mean {worst[0]:.3f} ulp (restatement {restated[0]:.3f}), var {worst[1]:.3f} ulp ({restated[1]:.3f})")
    record_error("posterior", orthogonal_mean_ulp=worst[0], orthogonal_var_ulp=worst[1], orthogonal_mean_ulp_restated=restated[0],
                 orthogonal_var_ulp_restated=restated[1])
    assert worst[0] <= 2.0 * restated[0] and worst[1] <= 2.0 * restated[1]


@pytest.mark.parametrize("name", ["width_f65_b1_x0", "gauss_f129_b1", "width_f16_b0_x0"])
def test_means_are_the_totals_of_explain(name):
    """wmf_explain_rows's out_total(u, i) is y~_i . x_u + beta_i as well.  Both calls on the same device buffers; the tolerance is
    the sum of both gates in absolute terms: this call's is relative to M (tests/posterior_ref.py), explain's to max_e |contrib(e)|,
    and an error of that size in each of the row's d contributions moves their sum by at most d max_e |contrib(e)|."""
    _lib, lib, _ptr, _stream = _api()
    c, ce = foldin_ref.case(name), explain_ref.case(name)
    for k in ("Y", "W32", "indptr", "indices", "values"):
        assert np.array_equal(c[k], ce[k])
    bufs = _upload(c)
    tg = np.array(ce["targets"])
    n, T, nnz, f = len(c["indptr"]) - 1, tg.shape[1], len(c["indices"]), c["f"]
    mean, _, fail = _score(c, tg, bufs=bufs)
    assert fail == 0
    ip, tg_d = _dev(c["indptr"], np.int64), _dev(np.append(tg.reshape(-1), 0), np.int32)
    contrib = torch.empty(nnz * T + 1, dtype=torch.float32, device="cuda")
    total = torch.empty(n * T, dtype=torch.float32, device="cuda")
    efail = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = int(lib.wmf_explain_workspace_bytes(n, f, T))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wmf_explain_rows(_ptr(bufs["Y"]), c["m"], f, c["ld"], c["bias"], _ptr(bufs["W"]), _ptr(ip), _ptr(bufs["indices"]),
                                    _ptr(bufs["values"]), n, _ptr(tg_d), T, _ptr(contrib), _ptr(total), _ptr(efail), _ptr(ws), need, _stream()))
    torch.cuda.synchronize()
    total = total.cpu().numpy().reshape(n, T).astype(np.float64)
    Yf = c["Y"][:, :f]
    m64, v64, M = ref.scores64(Yf, c["bias"], c["lam"], c["indptr"], c["indices"], c["values"], tg)
    m32, _ = ref.restated_scores32(Yf, c["bias"], c["W32"], c["indptr"], c["indices"], c["values"], tg)
    gate = ref.gate_of(ref.score_errors(m32, m64, M))
    worst = 0.0
    for u in range(n):
        lo, hi = int(c["indptr"][u]), int(c["indptr"][u + 1])
        for t in np.nonzero(tg[u] >= 0)[0]:
            if hi == lo:
                assert mean[u, t] == total[u, t]
                continue
            tol = gate[u, t] * M[u, t] + ce["gate"][u, t] * (hi - lo) * np.abs(ce["ref"][lo:hi, t]).max()
            worst = max(worst, abs(mean[u, t] - total[u, t]) / tol)
            assert abs(mean[u, t] - total[u, t]) <= tol, (name, u, t, mean[u, t], total[u, t], tol)
    print(f"{name}: |mean - explain's total|, worst difference / tolerance {worst:.3f}")
    record_error("posterior", **{name + "_mean_vs_explain_total_over_tol": worst})


# ---------------------------------------------------------------------------------------------------- 6. failures and refusals
def _indefinite_case(bad_value, without_row=False):
    """tests/test_gpu_foldin.py's: unit vectors as items and the identity as W_white, so the entry (item 3, bad_value) makes row 1's
    I + E_u = diag(.., 1 + bad_value, ..).  ld = f + 4: the rows have padding.  without_row: rows 0 and 2 only."""
    f, m, ld = 8, 8, 12
    rng = np.random.default_rng(3)
    Yf = foldin_ref.padded(np.eye(m, f, dtype=np.float32), ld)
    indptr = np.array([0, 3, 5, 9], dtype=np.int64)
    indices = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int32)
    values = rng.uniform(1, 5, 9).astype(np.float32)
    values[3] = bad_value
    if without_row:
        keep = np.r_[0:3, 5:9]
        indptr, indices, values = np.array([0, 3, 7], dtype=np.int64), indices[keep], values[keep]
    return dict(name="indefinite", f=f, ld=ld, bias=0, lam=0.0, m=m, Y=Yf, W32=foldin_ref.padded(np.eye(f, dtype=np.float32), ld), indptr=indptr,
                indices=indices, values=values)


def test_an_indefinite_row_is_reported_and_its_neighbours_are_untouched():
    tg = np.array([[0, 3, -1, 7]] * 3, dtype=np.int32)
    streams = np.array([4, 5, 6])
    good, fail = _draw(_indefinite_case(2.0), 17, SIGMA, streams=streams)
    gm, gv, sfail = _score(_indefinite_case(2.0), tg)
    assert fail == 0 and sfail == 0 and np.isfinite(good).all() and np.isfinite(gm).all()
    assert abs(gv[1, 1] - 1 / 3) <= 4 * 2.0 ** -23 and abs(gm[1, 1] - 1.0) <= 4 * 2.0 ** -23      # z = e_3 / sqrt 3, c_3 = 3 / sqrt 3
    without, _ = _draw(_indefinite_case(2.0, without_row=True), 17, SIGMA, streams=streams[[0, 2]])
    for bad_value in (-3.0, -2.0, -1.0):           # pivots 1 - 3 = -2, exactly -1, and exactly 0: each a failure
        c = _indefinite_case(bad_value)
        for n_draws in (17, 1):
            X, fail = _draw(c, n_draws, SIGMA, streams=streams)
            assert fail == 1, bad_value
            assert np.isnan(X[1, :, :8]).all() and (_bits(X[1, :, 8:]) == 0).all()
            for u, v in ((0, 0), (2, 1)):
                assert np.array_equal(_bits(X[u]), _bits(good[u, :n_draws])) and np.array_equal(_bits(X[u]), _bits(without[v, :n_draws]))
        mean, var, fail = _score(c, tg)
        assert fail == 1
        for out, ok in ((mean, gm), (var, gv)):
            assert np.isnan(out[1, [0, 1, 3]]).all() and _bits(out[1, 2:3])[0] == 0
            assert np.array_equal(_bits(out[[0, 2]]), _bits(ok[[0, 2]]))


def test_argument_errors_return_before_any_launch():
    _lib, lib, _ptr, _stream = _api()
    c = foldin_ref.case("width_f5_b0_x4")
    tg = ref.targets_for(c, 5)
    need = int(lib.wmf_posterior_draw_workspace_bytes(13, 5, 2))
    assert need >= 1 and need == int(lib.wmf_posterior_score_workspace_bytes(13, 5, 5))
    shared = [dict(f=0), dict(f=261), dict(ld=4), dict(ld=c["ld"] + 2), dict(m=0), dict(m=1 << 31), dict(n=-1), dict(n=1 << 31),
              dict(ws_bytes=need - 1)]
    shared += [{k: None} for k in ("Y", "W", "indptr", "indices", "values", "fail", "ws")]
    bad_draw = shared + [dict(n_draws=0), dict(n_draws=-3), dict(n_draws=ref.MAX_DRAWS + 1), dict(n=1 << 30), dict(sigma=-1.0),
                         dict(sigma=float("inf")), dict(sigma=float("nan")), dict(X=None)]
    for override in bad_draw:
        X, fail = _draw(c, 2, SIGMA, expect=_lib.WMF_EINVAL, args=override)
        assert (X == SENTINEL).all() and fail == 0, override
    bad_score = shared + [dict(n_targets=0), dict(n_targets=-3), dict(n_targets=ref.MAX_TARGETS + 1), dict(targets=None), dict(mean=None, var=None)]
    for override in bad_score:
        mean, var, fail = _score(c, tg, expect=_lib.WMF_EINVAL, args=override)
        assert (mean == SENTINEL).all() and (var == SENTINEL).all() and fail == 0, override
    X, fail = _draw(c, 2, SIGMA, args=dict(n=0))                                 # no rows: a no-op
    mean, var, sfail = _score(c, tg, args=dict(n=0))
    assert (X == SENTINEL).all() and (mean == SENTINEL).all() and (var == SENTINEL).all() and fail == sfail == 0


def test_which_kernels_ran():
    _lib, lib, _ptr, _stream = _api()
    c = foldin_ref.case("width_f5_b0_x4")
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    try:
        _draw(c, 2, SIGMA)
        _score(c, ref.targets_for(c, 5))
        _noise(1, None, np.arange(4), np.arange(4))
        torch.cuda.synchronize()
    finally:
        lib.wmf_profile_enable(0)
    table = {name: launches for name, _tag, _ms, launches, _lo, _hi in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    assert table == {"posterior_draw_kernel": 1, "posterior_score_kernel": 1, "posterior_noise_kernel": 1}
