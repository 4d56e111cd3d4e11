"""wmf_half_step_f64 through the C ABI (csrc/wmf_f64.hip, csrc/wmf_iter64.hip), PER ROW, against tests/f64_ref.py.

Every comparison is per row: ||got_u - ref_u|| / ||ref_u||, and a row without entries is compared with ==.  The gates:
    FORWARD      1e-10 for a row whose weights are all >= 0 -- the contract of include/wmf_hip.h
    FORWARD_NEG  1e-8 for a row with a weight below zero whose cond_2(A_u) <= 1e6 (the pivoted LU's rows)
    AGREE        1e-12 between the same row under two kernel-selection switches (the figure of tests/test_gpu_iter.py)
    ETA_GATE     the normwise backward error of the device's row, 3 x the worst measured on an MI355X
                 (profiles/r13_f64_rows.json; NumPy's float64 solve of the same systems leaves 4e-17 .. 1.5e-16)

WIDTHS is derived, not copied: route(f, flags) below restates the selection of wmf_launch_half_step_f64 and
wmf_launch_iter64 -- with f4 = ceil(f / 4), nb16 = ceil(f / 16),
    row solver     solve64v2_kernel<NB, TEAM, R> by nblk = f4 (f4 + 1) / 2 + f4: wave teams <1|2|3, 64, 8> while nblk <= 64 | 128 |
                   192 (f <= 36 | 56 | 72), workgroup teams <1|2|3|5|9, 256, 16> while nblk <= 256 | 512 | 768 | 1280 | beyond
                   (f <= 84 | 120 | 148 | 196 | 260)
    Gramian        gram64m_kernel<PW>, PW = ceil(nb16 (nb16 + 1) / 2 / 8) <= 6 (f <= 48 | 80 | 96 | 112 | 128 | 144), else -- and
                   under WMF_DBG_F64_VALU at every width -- gram64v2_kernel<NB> with NB by f4 (f4 + 1) / 2 <= 256 | 512 | 768 | 1280
                   (f <= 88 | 124 | 152 | 200 | 260); factor64_kernel<NB> with the same NB
    row transform  transform64m_kernel<KK, G> while 4 f4 x ldw doubles fit 160 KB (f <= 140: at f = 141 .. 144 they are 144 x 144),
                   KK = 16 | 17 | 20 | 24 | 28 | 32 | 33 | 36 for f <= 64 | 68 | 80 | 96 | 112 | 128 | 132 | 140; then
                   transform64_kernel<1>, <2> above f = 256
    iteration      solve64it_kernel<1, FPD, 8> and <4, FPD, NS>: FPD, NS = 4, 16 | 5, 12 | 8, 9 | 9, 9 for f <= 64 | 80 | 128 | 144,
                   none above
and WIDTHS is every f at which route(f) differs from route(f - 1) under any switch, with f - 1, plus the small widths (1 .. 5,
7, 8, 9: one and two 4-blocks, with and without padding), 16, 17 and 260.  test_route_of_every_width compares route() with the
launches the library records, so a change of the dispatch that this list does not follow fails there.

DEGREES: 0; 1 .. 5, 7, 8, 9 (the 4-entry blocks of the low-rank system, the 8-entry pass of the wave teams); 15, 16, 17 (the
16-entry pass of the workgroup teams and of the low-rank staging); 31, 32, 33, 34 (the low-rank switch); 64, 65; dmax - 1, dmax,
dmax + 1 for dmax = wmf_iter64_dmax(f) (256, 192, 144; 144 above f = 144 too); a row with a stored zero, one with a duplicated
column, one with every column of the fixed side twice, one of 5000 entries.  The fixed side has m = max(2 f, 64) + 7 rows,
uniform in [0, 1); lambda = 0.1; weights 10 log(1 + c), c = 1 .. 7.  Rows longer than m draw their columns with replacement.
With these weights tau_u ~ 7 d, so the iteration hands every row back; test_iteration_* scales the weights down.

Two mixes: MIX_A has exactly a quarter of its rows at 1 .. 32 entries (4 count == n: the low-rank path is on), MIX_B one filler
row more (4 count == n - 1: off, where nothing else forces it on -- without the iteration, that is at f > 144 or under
WMF_DBG_NO_ITER)."""
import functools

import numpy as np
import pytest
import torch

import f64_ref
from conftest import record_error

pytestmark = pytest.mark.gpu

LAMBDA = 0.1
FORWARD, FORWARD_NEG, AGREE = 1e-10, 1e-8, 1e-12
SENTINEL = -12345.0
NO_LOW_RANK, NO_ITER, VALU = 134217728, 268435456, 536870912
SWITCHES = {"default": 0, "no_low_rank": NO_LOW_RANK, "no_iter": NO_ITER, "valu": VALU}
# eta of the device's rows by the kernel family that solved them, (f <= 16, f > 16): 3 x the worst of profiles/r13_f64_rows.json
# -- measured 5.1e-15 | 1.7e-15 (direct: the 5000-entry row, one chain of 5000 sums per element), 3.0e-16 | 1.5e-16 (low-rank),
# 3.9e-16 | 1.4e-16 (iteration), 3.4e-16 | 1.2e-16 (pivoted LU).  Against NumPy's solve of the same rows of a case the worst
# ratios are 58 | 24 (direct), 6 | 4 (low-rank), 4 | 3 (iteration), 5.5 | 3.4 (pivoted LU).
ETA_GATE = {"direct": (1.5e-14, 5.2e-15), "low_rank": (9.1e-16, 4.4e-16), "iteration": (1.15e-15, 4.1e-16), "lu": (1.0e-15, 3.5e-16)}


def _eta_gate(family, f):
    return ETA_GATE[family][0 if f <= 16 else 1]


# ------------------------------------------------------------------------------------------------------------- the dispatch
def iter64_dmax(f):
    return 256 if f <= 64 else 192 if f <= 80 else 144 if f <= 144 else 0


def route(f, flags=0):
    """The kernels one half step launches at width f (names as the library's profile records them)."""
    f4, nb16 = (f + 3) // 4, (f + 15) // 16
    tri = f4 * (f4 + 1) // 2
    nb = 1 if tri <= 256 else 2 if tri <= 512 else 3 if tri <= 768 else 5 if tri <= 1280 else 9
    pw = (nb16 * (nb16 + 1) // 2 + 7) // 8
    valu = bool(flags & VALU)
    names = {"gram64v2_reduce_kernel", "rinv64_kernel", "solve64lr_kernel", "solve64_lu_kernel", f"factor64_kernel<{nb}>"}
    names.add(f"gram64m_kernel<{pw}>" if pw <= 6 and not valu else f"gram64v2_kernel<{nb}>")
    ldw = 16 * nb16 + (0 if nb16 & 1 else 16)
    if 4 * f4 * ldw * 8 <= 160 * 1024 and f4 <= 36 and not valu:
        kk = next(k for k, top in ((16, 16), (17, 17), (20, 20), (24, 24), (28, 28), (32, 32), (33, 33), (36, 36)) if f4 <= top)
        names.add(f"transform64m_kernel<{kk}, {2 if f4 <= 16 else 3}>")
    else:
        names.add(f"transform64_kernel<{1 if 4 * f4 <= 256 else 2}>")
    nblk = tri + f4
    for top, inst in ((64, "1, 64, 8"), (128, "2, 64, 8"), (192, "3, 64, 8"), (256, "1, 256, 16"), (512, "2, 256, 16"),
                      (768, "3, 256, 16"), (1280, "5, 256, 16"), (1 << 30, "9, 256, 16")):
        if nblk <= top:
            names.add(f"solve64v2_kernel<{inst}>")
            break
    if iter64_dmax(f) and not flags & (NO_ITER | NO_LOW_RANK):
        fpd, ns = (4, 16) if f <= 64 else (5, 12) if f <= 80 else (8, 9) if f <= 128 else (9, 9)
        names.update({f"solve64it_kernel<1, {fpd}, 8>", f"solve64it_kernel<4, {fpd}, {ns}>"})
    return frozenset(names)


def _derive_widths():
    edges = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 260}
    for f in range(2, 261):
        if any(route(f, s) != route(f - 1, s) for s in SWITCHES.values()):
            edges.update((f - 1, f))
    return sorted(edges)


WIDTHS = _derive_widths()
CASES = [(f, b) for f in WIDTHS for b in (0, 1) if f >= 2 or not b]
case = pytest.mark.parametrize("f,bias", CASES, ids=[f"f{f}-b{b}" for f, b in CASES])


# ------------------------------------------------------------------------------------------------------------------ helpers
def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _upload(Y, indptr, indices, values):
    return _dev(Y, np.float64), _dev(indptr, np.int64), _dev(np.append(indices, 0), np.int32), _dev(np.append(values, 0.0), np.float64)


def _run(dev, f, bias, lam=LAMBDA, flags=0, lo=0, n=None, want_fail=0):
    """One half step on rows [lo, lo + n) through a window of indptr; dev: _upload()'s buffers.  The output sits between
    sentinel rows and the workspace before guard bytes.  Returns X [n, f]."""
    _lib, lib, _ptr, _stream = _api()
    Yd, ipd, ixd, vd = dev
    m = Yd.shape[0]
    n = ipd.numel() - 1 - lo if n is None else n
    ws_bytes = int(lib.wmf_half_step_f64_workspace_bytes(f, m, n))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0x5A
    out = torch.full((n + 2, f), SENTINEL, dtype=torch.float64, device="cuda")
    fail = torch.zeros(4, dtype=torch.int32, device="cuda")
    fail[1:] = 77
    try:
        assert lib.wmf_debug_set_flags(flags) == 0
        _lib.check(lib.wmf_half_step_f64(_ptr(Yd), m, f, int(bias), _ptr(ipd[lo:]), _ptr(ixd), _ptr(vd), n, float(lam), _ptr(out[1:]),
                                         _ptr(ws), ws_bytes, _ptr(fail), _stream()))
        torch.cuda.synchronize()
    finally:
        lib.wmf_debug_set_flags(0)
    got = out.cpu().numpy()
    assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL), "a write outside the output rows"
    assert bool((ws[ws_bytes:] == 0x5A).all()), "a write past the workspace"
    assert fail.tolist() == [want_fail, 77, 77, 77], fail.tolist()
    return got[1:-1]


def _log_weights(rng, nnz):
    return 10 * np.log(1 + rng.integers(1, 8, nnz)).astype(np.float64)


def _fixed_side(f, bias, seed, m=None):
    m = max(2 * f, 64) + 7 if m is None else m
    Y = np.random.default_rng(seed).random((m, f))
    if bias:
        Y[:, 0] *= 0.5
    return Y


LOW = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32)
N_LOW = len(LOW) + 2                                                 # and the rows with a stored zero and with a duplicate


def _mix(f, m, seed):
    """(indptr, indices, values, labels) of MIX_B; MIX_A is its first n - 1 rows.  labels name the special rows."""
    rng = np.random.default_rng(seed)
    dmax = iter64_dmax(f) or 144
    deg = [0, *LOW, 33, 34, 64, 65, dmax - 1, dmax, dmax + 1, 6, 6, 2 * m, 5000]
    labels = {"stored_zero": len(deg) - 4, "duplicate": len(deg) - 3, "all_twice": len(deg) - 2}
    n = 4 * N_LOW + 1
    deg += [33 + (i % 8) for i in range(n - len(deg))]
    rows = [np.repeat(rng.permutation(m), 2) if u == labels["all_twice"] else rng.choice(m, d, replace=d > m) for u, d in enumerate(deg)]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    values = _log_weights(rng, indptr[-1])
    values[indptr[labels["stored_zero"]] + 2] = 0.0
    indices[indptr[labels["duplicate"]] + 4] = indices[indptr[labels["duplicate"]] + 1]
    assert 4 * sum(1 for d in deg if 1 <= d <= 32) == n - 1 and deg[-1] > 32
    return indptr, indices, values, labels


def _family(ref, lowrank_on):
    """The kernel family that solves each row the iteration does not take, by the kernels' own criteria: a row of 1 .. 32
    entries on the low-rank path goes to the pivoted LU when it has a weight below zero (E = sqrt(w) does not exist), any other
    row when its Cholesky meets a non-positive pivot, that is when A_u is not positive definite."""
    d = ref["degree"]
    low = lowrank_on & (d >= 1) & (d <= 32)
    fam = np.where(low, np.where(ref["neg"], "lu", "low_rank"), np.where(ref["pd"], "direct", "lu")).astype(object)
    fam[d == 0] = "empty"
    return fam


def _gate_rows(name, f, got, ref, c, fam):
    """The forward gate per row; returns the figures to record, eta of candidate c by family among them, and the eta checks
    [(name, family, eta)] for _assert_eta -- after record_error, so that a figure beyond its gate is still in the table."""
    err = f64_ref.row_errors(got, ref["x"])
    gate = np.where(ref["neg"], FORWARD_NEG, FORWARD)
    bad = np.flatnonzero(~(err <= gate))
    assert not bad.size, (name, [(int(u), int(ref["degree"][u]), float(err[u])) for u in bad[:8]])
    assert not got[ref["degree"] == 0].any(), (name, "a row without entries is not exactly 0")
    stats = {"forward": float(err.max())}
    for k in sorted(set(fam) - {"empty"}):
        sel = fam == k
        stats[f"eta_{k}"] = float(ref["eta"][c][sel].max())
        stats[f"eta_numpy_{k}"] = float(ref["eta_numpy"][sel].max())
    return stats, [(name, k, stats[f"eta_{k}"]) for k in sorted(set(fam) - {"empty"})]


def _assert_eta(checks, f):
    for name, family, eta in checks:
        assert eta <= _eta_gate(family, f), (name, family, eta, _eta_gate(family, f))


def _agree(name, outs):
    """Every pair of runs agrees to AGREE per row (rows of zeros: exactly)."""
    keys = list(outs)
    worst = 0.0
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            e = f64_ref.row_errors(outs[a], outs[b])
            assert np.all(e <= AGREE), (name, a, b, int(np.argmax(e)), float(e.max()))
            worst = max(worst, float(e.max()))
    return worst


# ------------------------------------------------------------------------------------------- every width, degree and switch
@case
def test_every_degree_under_every_switch(f, bias):
    Y = _fixed_side(f, bias, 1000 + 2 * f + bias)
    indptr, indices, values, labels = _mix(f, Y.shape[0], 77 + f)
    n_b = len(indptr) - 1
    dev = _upload(Y, indptr, indices, values)
    outs = {(mix, k): _run(dev, f, bias, flags=s, n=n) for mix, n in (("A", n_b - 1), ("B", n_b)) for k, s in SWITCHES.items()}
    # one reference for both mixes: a row is a function of its own entries, and MIX_A is MIX_B without its last row
    cands = [o if o.shape[0] == n_b else np.vstack([o, np.zeros((1, f))]) for o in outs.values()]
    ref_b = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values, candidates=cands)
    assert int(ref_b["neg"].sum()) == (1 if bias else 0)            # (the stored zero under a bias: w = -bias[idx] < 0)
    assert ref_b["neg"][labels["stored_zero"]] == bool(bias)
    iter_off = iter64_dmax(f) == 0
    stats, checks = {}, []
    for c, (mix, k) in enumerate(outs):
        n = outs[mix, k].shape[0]
        ref = {key: (v[:, :n] if key == "eta" else v[:n]) for key, v in ref_b.items()}
        s = SWITCHES[k]
        on = not s & NO_LOW_RANK and (mix == "A" or not (iter_off or s & NO_ITER))
        st, ch = _gate_rows(f"f{f}-b{bias}-{mix}-{k}", f, outs[mix, k], ref, c, _family(ref, on))
        stats.update({f"{mix}.{k}.{key}": v for key, v in st.items()})
        checks += ch
    for mix in "AB":
        stats[f"{mix}.agree"] = _agree(f"f{f}-b{bias}-{mix}", {k: outs[mix, k] for k in SWITCHES})
    # MIX_A, 4 count == n: the low-rank kernel takes its rows even without the iteration
    low = (ref_b["degree"][:-1] >= 1) & (ref_b["degree"][:-1] <= 32) & ~ref_b["neg"][:-1]
    differ = (outs["A", "no_iter"][low] != outs["A", "no_low_rank"][low]).any(axis=1)
    assert differ.mean() >= 0.5, "MIX_A: the low-rank kernel did not take its rows"
    # MIX_B, 4 count == n - 1: without the iteration the path is off -- the direct kernels, bit for bit
    assert np.array_equal(outs["B", "no_iter"], outs["B", "no_low_rank"])
    if iter_off:
        assert np.array_equal(outs["B", "default"], outs["B", "no_low_rank"])
    record_error(f"f64_rows[f={f},bias={bias}]", **stats)
    _assert_eta(checks, f)


def _launches(run):
    _lib, lib, _, _ = _api()
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        lib.wmf_profile_enable(0)
    table = {}
    for name, _tag, _ms, n, _lo, _hi in _lib.profile_table(lib):
        table[name] = table.get(name, 0) + int(n)
    lib.wmf_profile_reset()
    return table


def routing_table():
    """{switch: {width: kernels launched}} on a four-row matrix."""
    table = {}
    for k, s in SWITCHES.items():
        for f in WIDTHS:
            Y = _fixed_side(f, 0, f)
            indptr = np.array([0, 3, 3, 43, 48])
            rng = np.random.default_rng(f)
            dev = _upload(Y, indptr, rng.integers(0, Y.shape[0], 48), _log_weights(rng, 48))
            table.setdefault(k, {})[f] = _launches(lambda: _run(dev, f, 0, flags=s))
    return table


def test_route_of_every_width():
    """The launches the library records at every width and switch are route()'s -- the derivation of WIDTHS stands on the code --
    and between them the widths reach every instantiation the dispatch has."""
    table = routing_table()
    seen = set()
    for k, s in SWITCHES.items():
        for f in WIDTHS:
            got = table[k][f]
            assert set(got) == route(f, s), (k, f, sorted(set(got) ^ route(f, s)))
            assert all(c == (2 if name.startswith("transform64") else 1) for name, c in got.items()), (k, f, got)
            seen.update(got)
    every = set()
    for f in range(1, 261):
        for s in SWITCHES.values():
            every |= route(f, s)
    assert seen == every, sorted(every - seen)
    for name in ("solve64v2_kernel<2, 64, 8>", "solve64v2_kernel<1, 256, 16>", "solve64v2_kernel<5, 256, 16>", "gram64m_kernel<3>",
                 "gram64m_kernel<6>", "transform64m_kernel<17, 3>", "transform64m_kernel<20, 3>", "transform64m_kernel<24, 3>",
                 "transform64m_kernel<36, 3>", "transform64_kernel<2>", "solve64it_kernel<1, 5, 8>", "solve64it_kernel<4, 9, 9>"):
        assert name in seen, name
    assert route(72) >= {"solve64v2_kernel<3, 64, 8>"} and route(73) >= {"solve64v2_kernel<1, 256, 16>"}   # wave teams end at 72


# ---------------------------------------------------------------------------------------------------------------- iteration
ITER_WIDTHS = (16, 64, 65, 80, 81, 128, 129, 144)
TAUS = (0.01, 0.1, 0.3, 0.45, 0.49, 0.51, 0.7)
M_ITER = 307


@functools.lru_cache(maxsize=None)
def _iteration_case(f, bias):
    """Rows of 1, 8, 32, 33, 64, dmax, dmax + 1 entries, each at every tau of TAUS: the weights of a row are scaled so that the
    reference's tau_u lands there (with a bias the stored values are w + bias[idx], so that w is the scaled weight).  With a
    bias three more rows (8, 33, dmax entries, tau 0.1) carry ONE weight below zero."""
    Y = _fixed_side(f, bias, 5000 + f + bias, m=M_ITER)
    rng = np.random.default_rng(600 + f)
    dmax = iter64_dmax(f)
    plan = [(d, t, False) for d in (1, 8, 32, 33, 64, dmax, dmax + 1) for t in TAUS]
    if bias:
        plan += [(d, 0.1, True) for d in (8, 33, dmax)]
    deg = [p[0] for p in plan]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate([rng.choice(M_ITER, d, replace=False) for d in deg]).astype(np.int32)
    w = _log_weights(rng, indptr[-1])
    base = f64_ref.row_taus(f64_ref.tilde(Y, bias)[0], 0, LAMBDA, indptr, indices, w)   # tau of the weights themselves on Y~
    for u, (d, t, negative) in enumerate(plan):
        lo, hi = indptr[u], indptr[u + 1]
        w[lo:hi] *= t / base[u]
        if negative:
            w[lo + d // 2] *= -1.0
    values = w + Y[indices, 0] if bias else w
    assert 4 * sum(1 for d in deg if d <= 32) >= len(deg)
    for a in (Y, indptr, indices, values):
        a.setflags(write=False)
    return Y, indptr, indices, values, plan


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("f", ITER_WIDTHS)
def test_iteration_on_both_sides_of_tau(f, bias):
    """The series (tau 0.01, 0.1), the Chebyshev recurrence (0.3 .. 0.49) and the hand-back (0.51, 0.7; dmax + 1 entries; a weight
    below zero): every row meets the forward gate whichever kernel took it.  There is no counter on this path; that the
    iteration ran shows in the bits: of the rows with tau <= 0.4 and no negative weight at least half differ from the same
    run under WMF_DBG_NO_ITER, and every row the iteration must hand back is bit-identical to that run."""
    Y, indptr, indices, values, plan = _iteration_case(f, bias)
    dev = _upload(Y, indptr, indices, values)
    outs = {k: _run(dev, f, bias, flags=s) for k, s in SWITCHES.items()}
    ref = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values, candidates=list(outs.values()))
    want_tau = np.array([p[1] for p in plan])
    assert np.all(np.abs(ref["tau"] - want_tau) <= 1e-6 * want_tau), np.abs(ref["tau"] / want_tau - 1).max()
    assert np.array_equal(ref["neg"], np.array([p[2] for p in plan]))
    dmax = iter64_dmax(f)
    solved = (ref["tau"] <= 0.4) & ~ref["neg"]                      # (the issue's set: its rows of dmax + 1 entries cannot differ)
    back = (ref["tau"] >= 0.51) | ref["neg"] | (ref["degree"] > dmax)
    stats, checks = {}, []
    for c, k in enumerate(SWITCHES):
        fam = _family(ref, k != "no_low_rank")
        if k in ("default", "valu"):
            fam[~back & ~ref["neg"]] = "iteration"
        st, ch = _gate_rows(f"iter-f{f}-b{bias}-{k}", f, outs[k], ref, c, fam)
        stats.update({f"{k}.{key}": v for key, v in st.items()})
        checks += ch
    stats["agree"] = _agree(f"iter-f{f}-b{bias}", outs)
    differ = (outs["default"] != outs["no_iter"]).any(axis=1)
    stats["solved_rows_that_differ"] = float(differ[solved].mean())
    record_error(f"f64_iteration[f={f},bias={bias}]", **stats)
    _assert_eta(checks, f)
    assert differ[solved].mean() >= 0.5, differ[solved].mean()
    assert not differ[back].any(), [plan[u] for u in np.flatnonzero(differ & back)]


# --------------------------------------------------------------------------------------------------- a sharp case, in ulps
ULPS_DIRECT, ULPS_LOW_RANK = 7, 18


def _sharp_case(f):
    """A fixed side of signed unit vectors scaled by powers of two: column c has class p = 1 + c % 3 and, for q = 0 .. p - 1,
    three rows +-2^q e_c, so G_cc = 3 (1 + 4 + .. + 4^(p-1)) = 4^p - 1 and with lambda = 1 the regularised Gramian is
    diag(4^p), exactly, in any order of summation.  A row hits DISTINCT columns (one of the column's rows each; its first entry a
    row of the top scale, weights k / 4 >= 4, so that tau_u >= 1 and the iteration hands the row back): A_u is diagonal,
    every sum has one non-zero term, and x_c = s 2^q (w + 1) / (4^p + w 4^q) for a hit column, 0 elsewhere."""
    rng = np.random.default_rng(f)
    rows = [(c, q, 1.0 if (c + q + r) % 2 else -1.0) for c in range(f) for q in range(1 + c % 3) for r in range(3)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    Y = np.zeros((len(rows), f))
    by_col = {}
    for j, (c, q, sgn) in enumerate(rows):
        Y[j, c] = sgn * 2.0 ** q
        by_col.setdefault(c, []).append(j)
    deg = sorted({min(f, d) for d in (1, 2, 5, 32, 33, 40, f)})
    indices, values, want = [], [], np.zeros((len(deg), f), dtype=object)
    from fractions import Fraction
    for u, d in enumerate(deg):
        for i, c in enumerate(rng.choice(f, d, replace=False)):
            cands = by_col[int(c)]
            if i == 0:
                cands = [j for j in cands if rows[j][1] == c % 3]
            j = int(rng.choice(cands))
            w = Fraction(int(rng.integers(16, 161)), 4)
            _, q, sgn = rows[j]
            indices.append(j)
            values.append(float(w))
            want[u, c] = Fraction(sgn) * 2 ** q * (w + 1) / (4 ** (1 + c % 3) + w * 4 ** q)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return Y, indptr, np.array(indices, dtype=np.int32), np.array(values), want


@pytest.mark.parametrize("f", WIDTHS)
def test_diagonal_systems_to_the_ulp(f):
    """Elementwise, in ulps of the exact quotient (fractions.Fraction), under every switch.  The gate is the number of
    operations that can round on the way to one element -- each moves the element by at most half an ulp, also where its
    result is used twice, so the count bounds the error with room to spare:
      direct kernels (solve64v2_kernel), 7: p = w + 1; A_cc = w y^2 + G_cc (w y, (w y) y and the sums with zeros are exact: y is
        a power of two); the last Newton step of f64_rsqrt (x y, the residual, the update: the steps before it are contracted
        away); R^-T b; R^-1 y.
      low-rank form (rows of 1 .. 32 entries), 18: f64_rsqrt of G_cc in factor64_kernel (3; rinv64_kernel and both
        transforms only scale by it or by powers of two); sqrt(w); p = w + 1 and p / sqrt(w); S_ee = v v; P_ee = e S e + 1 (3);
        f64_rsqrt of P_ee (3); R^-T t; R^-1 y; c = e y; g = v c; x = g R^-1_cc.
    A column that is not hit is exactly 0.  What this sees and the 1e-10 gates cannot: a dropped or misplaced column in the
    padding of f % 4 != 0, a lost low-order part anywhere."""
    from fractions import Fraction
    Y, indptr, indices, values, want = _sharp_case(f)
    dev = _upload(Y, indptr, indices, values)
    deg = np.diff(indptr)
    assert 4 * int((deg <= 32).sum()) >= len(deg)
    outs = {k: _run(dev, f, 0, lam=1.0, flags=s) for k, s in SWITCHES.items()}
    assert np.array_equal(outs["default"], outs["no_iter"])          # tau_u >= 1: every row is handed back
    worst = {}
    for k, got in outs.items():
        for u in range(len(deg)):
            gate = ULPS_LOW_RANK if deg[u] <= 32 and k != "no_low_rank" else ULPS_DIRECT
            for c in range(f):
                if want[u, c] == 0:
                    assert got[u, c] == 0.0, (k, u, c, got[u, c])
                    continue
                ulp = Fraction(float(np.spacing(abs(float(want[u, c])))))
                off = float(abs(Fraction(float(got[u, c])) - want[u, c]) / ulp)
                fam = "low_rank" if gate == ULPS_LOW_RANK else "direct"
                worst[fam] = max(worst.get(fam, 0.0), off)
                assert off <= gate, (k, u, int(deg[u]), c, off)
    record_error(f"f64_sharp[f={f}]", **{f"ulps_{k}": v for k, v in worst.items()})


# ----------------------------------------------------------------------------------------------- negative weights: pivoted LU
def _negative_case(f, n, seed):
    m = max(2 * f, 64) + 7
    rng = np.random.default_rng(seed)
    Y = rng.random((m, f))
    Y[:, 0] = np.linspace(-5, 30, m)
    deg = rng.integers(1, 81, n)
    deg[:4] = (0, 1, 32, 33)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate([rng.choice(m, d, replace=d > m) for d in deg]).astype(np.int32)
    return Y, indptr, indices, _log_weights(rng, indptr[-1])


@pytest.mark.parametrize("f", [2, 5, 16, 37, 65, 85, 129, 197])
def test_indefinite_rows_through_the_pivoted_kernel(f):
    """A bias column of linspace(-5, 30): about nine rows in ten have a weight below zero; the share of systems that are not
    positive definite is recorded (0.02 at f = 2, 0.58 at f = 5, above 0.9 from f = 16 on).  Forward 1e-8 (1e-10 without a negative weight) on the rows with cond <= 1e6 -- which must be >= 95 %
    of the rows --, eta on EVERY row, by the family that solves it (_family)."""
    Y, indptr, indices, values = _negative_case(f, 48 if f <= 128 else 32, 900 + f)
    dev = _upload(Y, indptr, indices, values)
    outs = {k: _run(dev, f, 1, flags=s) for k, s in SWITCHES.items()}
    ref = f64_ref.half_step(Y, 1, LAMBDA, indptr, indices, values, candidates=list(outs.values()), want_cond=True)
    assert ref["neg"].mean() >= 0.6
    assert 4 * int(((ref["degree"] >= 1) & (ref["degree"] <= 32)).sum()) >= len(ref["degree"])   # the low-rank path is on
    tame = ~(ref["cond"] > 1e6)
    assert tame.mean() >= 0.95, tame.mean()
    stats = {"worst_cond": float(np.nanmax(ref["cond"])), "not_positive_definite": float((~ref["pd"]).mean())}
    gates = []
    for c, k in enumerate(SWITCHES):
        err = f64_ref.row_errors(outs[k], ref["x"])
        gate = np.where(ref["neg"], FORWARD_NEG, FORWARD)
        assert np.all(err[tame] <= gate[tame]), (k, int(np.argmax(np.where(tame, err / gate, 0))), float(err[tame].max()))
        assert not outs[k][0].any()
        stats[f"{k}.forward"] = float(err[tame].max())
        fam = _family(ref, k != "no_low_rank")
        for name in sorted(set(fam) - {"empty"}):
            stats[f"{k}.eta_{name}"] = float(ref["eta"][c][fam == name].max())
            stats[f"{k}.eta_numpy_{name}"] = float(ref["eta_numpy"][fam == name].max())
            gates.append((k, name, stats[f"{k}.eta_{name}"]))
    record_error(f"f64_indefinite[f={f}]", **stats)
    for k, name, eta in gates:                                      # every row, those beyond cond 1e6 too
        assert eta <= _eta_gate(name, f), (k, name, eta)


def test_more_fallback_rows_than_the_pivoted_kernels_grid_twice():
    """600 rows of which far more than WMF_F64_LU_GRID = 256 reach the fallback list -- counted on the host by the kernels' own
    criteria (_family) and asserted with a margin --, so that workgroups of solve64_lu_kernel take a second and a third row.  The
    order of the list is decided by atomics, the rows may not depend on it: three runs, bit for bit."""
    f, n = 5, 600
    Y, indptr, indices, values = _negative_case(f, n, 31)
    dev = _upload(Y, indptr, indices, values)
    first = _run(dev, f, 1)
    ref = f64_ref.half_step(Y, 1, LAMBDA, indptr, indices, values, candidates=[first], want_cond=True)
    fam = _family(ref, True)
    listed = int((fam == "lu").sum())
    assert listed >= 256 + 64, listed
    tame = ~(ref["cond"] > 1e6)
    assert tame.mean() >= 0.95
    err = f64_ref.row_errors(first, ref["x"])
    assert np.all(err[tame] <= np.where(ref["neg"], FORWARD_NEG, FORWARD)[tame]), float(err[tame].max())
    stats = {f"eta_{k}": float(ref["eta"][0][fam == k].max()) for k in sorted(set(fam) - {"empty"})}
    record_error("f64_indefinite[f=5,n=600]", forward=float(err[tame].max()), fallback_rows=listed, **stats)
    for k in sorted(set(fam) - {"empty"}):
        assert stats[f"eta_{k}"] <= _eta_gate(k, f), (k, stats[f"eta_{k}"])
    for _ in range(2):
        assert np.array_equal(first, _run(dev, f, 1))


# ---------------------------------------------------------------------------------------------------------------- grid caps
def _short_rows(n, m, seed, lo=1, hi=6):
    rng = np.random.default_rng(seed)
    deg = rng.integers(lo, hi + 1, n)
    deg[[0, n // 2, n - 1]] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return indptr, rng.integers(0, m, indptr[-1]).astype(np.int32), _log_weights(rng, indptr[-1])


@pytest.mark.parametrize("f,n,batch", [(16, 4 * 4096 + 5, 2048), (85, 4096 + 3, 256)])
def test_more_rows_than_the_row_solvers_grid(f, n, batch):
    """Four rows per workgroup of the wave-team solver and of solve64lr_kernel (f = 16), one per workgroup of the
    workgroup-team solver (f = 85), 4096 workgroups at the most: the last rows are reached in a second trip."""
    Y = _fixed_side(f, 0, f)
    indptr, indices, values = _short_rows(n, Y.shape[0], f)
    want = f64_ref.half_step_batched(Y, 0, LAMBDA, indptr, indices, values, batch=batch)
    dev = _upload(Y, indptr, indices, values)
    for k in ("no_low_rank", "no_iter") if f == 16 else ("no_low_rank",):
        got = _run(dev, f, 0, flags=SWITCHES[k])
        err = f64_ref.row_errors(got, want)
        record_error(f"f64_grid_cap[f={f},n={n},{k}]", forward=float(err.max()))
        assert np.all(err <= FORWARD), (k, int(np.argmax(err)), float(err.max()))


@pytest.mark.parametrize("n,lo,hi", [(4 * 4096 + 5, 1, 6), (4096 + 3, 33, 36)])
def test_more_rows_than_the_iterations_grid(n, lo, hi):
    """solve64it_kernel: 4096 workgroups of four one-wave teams (rows of 1 .. 32 entries) or of one four-wave team (33 and more).
    f = 16 under the default switches, the weights scaled by 1e-3 so that tau_u <= 36 * 0.021 * max_e y~^T (G~ + lambda I)^-1 y~
    stays far below the bound (asserted <= 0.4): every row is the iteration's, the last ones in a second trip; that it took them
    shows in their bits against the run without it."""
    f = 16
    Y = _fixed_side(f, 0, f)
    indptr, indices, values = _short_rows(n, Y.shape[0], n, lo, hi)
    values = 1e-3 * values
    assert f64_ref.row_taus(Y, 0, LAMBDA, indptr, indices, values).max() <= 0.4
    want = f64_ref.half_step_batched(Y, 0, LAMBDA, indptr, indices, values, batch=512)
    dev = _upload(Y, indptr, indices, values)
    got, direct = _run(dev, f, 0), _run(dev, f, 0, flags=NO_ITER)
    for k, x in (("default", got), ("no_iter", direct)):
        err = f64_ref.row_errors(x, want)
        record_error(f"f64_grid_cap[f={f},n={n},iteration,{k}]", forward=float(err.max()))
        assert np.all(err <= FORWARD), (k, int(np.argmax(err)), float(err.max()))
    tail = np.flatnonzero(np.diff(indptr) > 0)
    tail = tail[tail >= (4 * 4096 if hi <= 32 else 4096)]
    assert tail.size and (got[tail] != direct[tail]).any(axis=1).all(), "the rows past the grid were not the iteration's"
    assert (got != direct).any(axis=1).mean() >= 0.5


def test_more_rows_than_the_counting_kernels_grid():
    """f64_count_low_kernel: 1024 workgroups of 256 threads.  262 144 + 300 rows, the rows with entries (1 .. 3 each) exactly a
    quarter of them and the last 300 among these: without the iteration the low-rank path is on if and only if the count saw
    the tail -- then its rows differ in bits from the direct kernels' --, and with one such row emptied it is off."""
    f, n = 4, 262144 + 300
    Y = _fixed_side(f, 0, 4)
    rng = np.random.default_rng(8)
    deg = np.zeros(n, dtype=np.int64)
    quarter = (n + 3) // 4
    assert 4 * quarter == n
    rows = np.concatenate([rng.choice(n - 300, quarter - 300, replace=False), np.arange(n - 300, n)])
    deg[rows] = rng.integers(1, 4, quarter)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, Y.shape[0], indptr[-1]).astype(np.int32)
    values = _log_weights(rng, indptr[-1])
    want = f64_ref.half_step_batched(Y, 0, LAMBDA, indptr, indices, values, batch=65536)
    dev = _upload(Y, indptr, indices, values)
    direct, low = _run(dev, f, 0, flags=NO_LOW_RANK), _run(dev, f, 0, flags=NO_ITER)
    for got in (direct, low):
        err = f64_ref.row_errors(got, want)
        assert np.all(err <= FORWARD), (int(np.argmax(err)), float(err.max()))
    assert (direct[rows] != low[rows]).any(axis=1).mean() >= 0.5
    # one row fewer: its entries go to the row before it (which had entries: it stays at 1 .. 32)
    last = int(np.flatnonzero(deg)[-1])
    assert deg[last - 1] > 0
    ip2 = indptr.copy()
    ip2[last] = ip2[last + 1]
    dev2 = _upload(Y, ip2, indices, values)
    assert np.array_equal(_run(dev2, f, 0, flags=NO_ITER), _run(dev2, f, 0, flags=NO_LOW_RANK))


@pytest.mark.parametrize("f,m,precise", [(65, 32768 + 17, True), (5, 131072 + 300, True), (145, 131072 + 300, False)])
def test_a_fixed_side_longer_than_the_dense_kernels_grids(f, m, precise):
    """transform64m_kernel: 256 workgroups x 8 waves x 16 rows per trip (f = 65); gram64m_kernel: 512 workgroups of 256 rows
    and more (f = 5); transform64_kernel: 2048 workgroups (f = 145, VALU forms).  Rows whose entries lie in the last rows of the
    fixed side, where a trip that is cut short shows; small weights, so that at f = 65 the iteration takes the longer rows."""
    Y = _fixed_side(f, 1, f, m=m)
    rng = np.random.default_rng(m)
    deg = np.array([0, 1, 4, 17, 32, 33, 40, 64, 3, 9])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate([rng.choice(np.arange(m - 300, m), d, replace=False) for d in deg]).astype(np.int32)
    indices[indptr[3]] = m - 1
    values = 0.05 * _log_weights(rng, indptr[-1]) + 0.5              # (above every bias: no weight below zero)
    dev = _upload(Y, indptr, indices, values)
    outs = {k: _run(dev, f, 1, flags=s) for k, s in SWITCHES.items()}
    ref = f64_ref.half_step(Y, 1, LAMBDA, indptr, indices, values, candidates=list(outs.values()), gram_precise=precise)
    assert not ref["neg"].any()
    for k in outs:
        err = f64_ref.row_errors(outs[k], ref["x"])
        record_error(f"f64_long_fixed_side[f={f},{k}]", forward=float(err.max()))
        assert np.all(err <= FORWARD), (k, int(np.argmax(err)), float(err.max()))
    _agree(f"long-fixed-side-f{f}", outs)


# ----------------------------------------------------------------------------------------------------------- contract edges
def test_no_rows():
    Y = _fixed_side(5, 0, 1)
    dev = _upload(Y, np.array([0]), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert _run(dev, 5, 0).shape == (0, 5)


@pytest.mark.parametrize("f,bias", [(1, 0), (5, 1), (65, 0), (145, 1)])
def test_a_fixed_side_of_one_row(f, bias):
    Y = (np.random.default_rng(f).random((1, f)) + 0.25) / np.sqrt(f)
    indptr = np.array([0, 1, 1, 3, 40])
    indices = np.zeros(40, dtype=np.int32)
    values = _log_weights(np.random.default_rng(1), 40)
    dev = _upload(Y, indptr, indices, values)
    outs = {k: _run(dev, f, bias, flags=s) for k, s in SWITCHES.items()}
    ref = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values, want_cond=True)
    # G~ has rank one: cond(A_u) = 1 + ||y~||^2 (1 + sum w) / lambda with ||y||^2 <= 1.6 and sum w <= 37 * 21
    assert np.nanmax(ref["cond"]) <= 3e4
    for k in outs:
        err = f64_ref.row_errors(outs[k], ref["x"])
        assert np.all(err <= FORWARD), (k, err)


@pytest.mark.parametrize("lo,n", [(0, 9), (2, 5), (8, 1), (3, 0), (1, 8)])
def test_indptr_windows(lo, n):
    """Rows [lo, lo + n) of a longer CSR: indptr[0] > 0, the window's pointers index the whole index and value arrays."""
    f, bias = 37, 1
    Y = _fixed_side(f, bias, 3)
    rng = np.random.default_rng(12)
    deg = np.array([5, 0, 33, 1, 32, 64, 0, 9, 40])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, Y.shape[0], indptr[-1]).astype(np.int32)
    values = _log_weights(rng, indptr[-1])
    ref = f64_ref.half_step(Y, bias, LAMBDA, indptr, indices, values)
    dev = _upload(Y, indptr, indices, values)
    for k, s in SWITCHES.items():
        got = _run(dev, f, bias, flags=s, lo=lo, n=n)
        err = f64_ref.row_errors(got, ref["x"][lo: lo + n])
        assert np.all(err <= FORWARD), (k, err)


def test_an_exactly_singular_row_is_counted_and_nan():
    """f = 2, lambda = 0 and a fixed side whose second column is zero: every system with entries is exactly singular in its
    second unknown -- except that a row WITHOUT entries is 0 by definition.  With one row of entries: fail_count == 1, that row
    NaN, the empty rows exactly 0; the synchronous host call answers WMF_ENUMERIC."""
    _lib, lib, _ptr, _stream = _api()
    Y = np.zeros((9, 2))
    Y[:, 0] = np.arange(1.0, 10.0)
    indptr = np.array([0, 0, 3, 3])
    indices = np.array([1, 4, 7], dtype=np.int32)
    values = np.array([2.0, 3.0, 1.0])
    dev = _upload(Y, indptr, indices, values)
    for s in SWITCHES.values():
        got = _run(dev, 2, 0, lam=0.0, flags=s, want_fail=1)
        assert np.isnan(got[1]).all() and not got[0].any() and not got[2].any()
    X = np.zeros((3, 2))
    ip, ix, v = indptr.astype(np.int64), indices, values
    rc = lib.wmf_recompute_factors_f64_host(Y.ctypes.data, 9, 2, 0, ip.ctypes.data, ix.ctypes.data, v.ctypes.data, 3, 0.0, X.ctypes.data)
    assert rc == _lib.WMF_ENUMERIC
    # the same rows with lambda > 0 are regular: the status belongs to the system, not to the call
    ok = _run(dev, 2, 0, lam=0.5)
    ref = f64_ref.half_step(Y, 0, 0.5, indptr, indices, values)
    assert np.all(f64_ref.row_errors(ok, ref["x"]) <= FORWARD)


def test_bad_arguments_are_refused_before_any_launch():
    _lib, lib, _ptr, _stream = _api()
    f, m, n = 5, 20, 3
    Y = _fixed_side(f, 0, 1, m=m)
    indptr = np.array([0, 2, 2, 5])
    Yd, ipd, ixd, vd = _upload(Y, indptr, np.arange(5), np.ones(5))
    need = int(lib.wmf_half_step_f64_workspace_bytes(f, m, n))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((n, f), SENTINEL, dtype=torch.float64, device="cuda")
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(Y=_ptr(Yd), m=m, f=f, indptr=_ptr(ipd), indices=_ptr(ixd), values=_ptr(vd), X=_ptr(out), ws=_ptr(ws), bytes=need,
                 fail=_ptr(fail))
        a.update(kw)
        return lib.wmf_half_step_f64(a["Y"], a["m"], a["f"], 0, a["indptr"], a["indices"], a["values"], n, LAMBDA, a["X"], a["ws"],
                                     a["bytes"], a["fail"], _stream())
    # (indices and values may be null: a matrix without entries has none, and the call cannot read indptr to know)
    bad = [dict(f=0), dict(f=261), dict(m=0), dict(bytes=need - 1)] + [{k: None} for k in ("Y", "indptr", "X", "ws", "fail")]
    for kw in bad:
        assert call(**kw) == _lib.WMF_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(fail[0]) == 0      # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


if __name__ == "__main__":
    import pprint
    table = routing_table()
    print("WIDTHS = " + repr(WIDTHS))
    names = {}
    for k in table:
        for f, got in table[k].items():
            for name in got:
                names.setdefault(name, {}).setdefault(k, []).append(f)
    print("ROUTES = " + pprint.pformat(names, width=150, compact=True))
