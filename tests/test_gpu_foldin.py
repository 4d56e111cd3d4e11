"""wmf_foldin_rows through the C ABI: every live row within its gate of the float64 definition (tests/foldin_ref.py: the gate of a
row is 4 x the error of the float32 restatement on that row + 8 ulps) at every width and layout of the serving tests, every
row-length edge and input family, a 9000-entry row and more rows than workgroups; padding, sentinels, indptr windows,
determinism and independence of rows; the exactly orthogonal catalogue against fractions.Fraction; the scores of the folded-in
row against wmf_explain_rows's totals; the failure report and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref
import foldin_ref as ref
from conftest import record_error

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64


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


def _foldin(c, first=0, count=None, expect=0, bufs=None, **override):
    """Rows [first, first + count) of case c through an indptr window.  Returns (X [count, ld], fail count); the guards around the
    output, the failure counter and the workspace are checked here, and with expect != 0 that nothing at all was written."""
    _lib, lib, _ptr, _stream = _api()
    n_all = len(c["indptr"]) - 1
    count = n_all - first if count is None else count
    d = bufs or _upload(c)
    ip = _dev(c["indptr"][first:first + count + 1], np.int64)
    X = torch.full((count * c["ld"] + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    fail = torch.tensor([-7, 0, -7], dtype=torch.int32, device="cuda")
    need = int(lib.wmf_foldin_workspace_bytes(count, c["f"]))
    ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    args = dict(Y=_ptr(d["Y"]), m=c["m"], f=c["f"], ld=c["ld"], bias=c["bias"], W=_ptr(d["W"]), indptr=_ptr(ip), indices=_ptr(d["indices"]),
                values=_ptr(d["values"]), n=count, X=ctypes.c_void_p(X.data_ptr() + 4 * GUARD), fail=ctypes.c_void_p(fail.data_ptr() + 4),
                ws=_ptr(ws), ws_bytes=need)
    args.update(override)
    rc = lib.wmf_foldin_rows(args["Y"], args["m"], args["f"], args["ld"], args["bias"], args["W"], args["indptr"], args["indices"],
                             args["values"], args["n"], args["X"], args["fail"], args["ws"], args["ws_bytes"], _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.wmf_last_error())
    xh, fh = X.cpu().numpy(), fail.cpu().numpy()
    assert (xh[:GUARD] == SENTINEL).all() and (xh[-GUARD:] == SENTINEL).all(), "X_out guards"
    assert fh[0] == -7 and fh[2] == -7, "fail_count guards"
    assert (ws.cpu().numpy() == 0x5A).all(), "the workspace is reserved, not written"
    return xh[GUARD:-GUARD].reshape(count, c["ld"]), int(fh[1])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_against_reference(c, X, first=0):
    """Every element written, the padding exactly zero, empty rows exactly zero, every live row within its gate; returns the row
    errors."""
    n, f = X.shape[0], c["f"]
    assert not (X == SENTINEL).any(), "an output element was not written"
    assert (_bits(X[:, f:]) == 0).all(), "the padding columns are not +0.0"
    live = c["live"][first:first + n]
    assert (_bits(X[~live]) == 0).all(), "an empty row is not zero"
    assert np.isfinite(X).all()
    err = ref.row_errors(X[:, :f], c["ref"][first:first + n])
    gate = c["gate"][first:first + n]
    bad = live & (err > gate)
    assert not bad.any(), (c["name"], [(int(u) + first, float(err[u]), float(gate[u])) for u in np.nonzero(bad)[0]][:5])
    return np.where(live, err, 0.0)


@pytest.mark.parametrize("name", ref.case_names())
def test_rows(name):
    """Widths 1 .. 260 and their leading dimensions, f = 30 .. 32, the six weight families at the four family widths, degrees
    0 .. 3, 7 .. 9, f - 1 .. f + 1 and 33 with empty rows first, in the middle and last, the 9000-entry row, 1030 rows at f = 8."""
    c = ref.case(name)
    X, fail = _foldin(c)
    assert fail == 0
    err = _check_against_reference(c, X)
    u = int(err.argmax())
    record_error("foldin_rows", **{name: err.max(), name + "_restated": c["restated_err"].max(),
                                   name + "_worst_row_degree": int(c["indptr"][u + 1] - c["indptr"][u])})


@pytest.mark.parametrize("name", ["width_f65_b1_x0", "width_f260_b0_x12", "width_f5_b0_x4"])
def test_indptr_window_and_row_counts(name):
    """A window starting at row 2, three rows, one row: the bits of the full launch; nothing outside the window's rows is written
    (the guards of _foldin lie directly around them)."""
    c = ref.case(name)
    full, _ = _foldin(c)
    for first, count in ((2, None), (5, 3), (9, 1), (4, 1)):
        X, fail = _foldin(c, first, count)
        assert fail == 0 and np.array_equal(_bits(X), _bits(full[first:first + X.shape[0]]))
    _check_against_reference(c, _foldin(c, 2)[0], first=2)


def test_two_runs_a_row_alone_and_another_position_give_the_same_bits():
    c = ref.case("width_f129_b1_x0")
    a, _ = _foldin(c)
    b, _ = _foldin(c)
    assert np.array_equal(_bits(a), _bits(b))
    alone, _ = _foldin(c, 10, 1)
    assert np.array_equal(_bits(alone[0]), _bits(a[10]))
    # rows 10 and 3 of the case as rows 0 and 1 of another CSR
    ip = c["indptr"]
    rows = (10, 3)
    moved = dict(c)
    moved["indices"] = np.concatenate([c["indices"][ip[r]:ip[r + 1]] for r in rows])
    moved["values"] = np.concatenate([c["values"][ip[r]:ip[r + 1]] for r in rows])
    moved["indptr"] = np.concatenate([[0], np.cumsum([ip[r + 1] - ip[r] for r in rows])]).astype(np.int64)
    m, _ = _foldin(moved)
    for k, r in enumerate(rows):
        assert np.array_equal(_bits(m[k]), _bits(a[r]))


def test_orthogonal_catalogue_against_fractions():
    """Items are scaled unit vectors: the components on axes the history does not touch are exactly 0.0, the others within 2 x
    the worst ulp error of the float32 restatement against the closed form in exact rational arithmetic."""
    c, exact = ref.orthogonal_exact()
    bound, measured = ref.orthogonal_ulp_bound()
    X, fail = _foldin(c)
    assert fail == 0
    worst = 0.0
    for u in range(X.shape[0]):
        for a in range(c["f"]):
            if (u, a) in exact:
                worst = max(worst, ref.ulp_error(X[u, a], exact[(u, a)]))
            else:
                assert X[u, a] == 0.0
    print(f"orthogonal catalogue: device {worst:.3f} ulp, restatement {measured:.3f} ulp, bound {bound:.3f} ulp")
    record_error("foldin_rows", orthogonal_ulp=worst, orthogonal_ulp_restated=measured)
    assert worst <= bound


@pytest.mark.parametrize("name", ["width_f65_b1_x0", "gauss_f129_b1", "width_f16_b0_x0"])
def test_scores_of_the_folded_in_row_are_the_totals_of_explain(name):
    """wmf_explain_rows documents out_total(u, i) as y~_i . x_u + beta_i.  Both calls on the same device buffers; the score is
    taken in float64 from the device's x.  Tolerance: the sum of the two calls' gates, both taken relative to one magnitude M
    that bounds what either gate is relative to, carried over to a score: the fold-in's gate is relative to max_a |x_a|, and an
    error of that size in every component moves the score by at most |y~_i|_1 max_a |x_a|; explain's gate is relative to
    max_e |contrib(e)|, and an error of that size in each of the row's d contributions moves their sum by at most
    d max_e |contrib(e)|.  M = the larger of the two, from the float64 references."""
    _lib, lib, _ptr, _stream = _api()
    c, ce = ref.case(name), explain_ref.case(name)
    for k in ("Y", "W32", "indptr", "indices", "values"):
        assert np.array_equal(c[k], ce[k])                          # the same inputs under the same name
    bufs = _upload(c)
    X, fail = _foldin(c, bufs=bufs)
    assert fail == 0
    n, T, nnz = len(c["indptr"]) - 1, ce["targets"].shape[1], len(c["indices"])
    ip, tg = _dev(c["indptr"], np.int64), _dev(np.append(ce["targets"].reshape(-1), 0), np.int32)
    contrib = torch.empty(nnz * T + 1, dtype=torch.float32, device="cuda")
    total = torch.empty(n * T, dtype=torch.float32, device="cuda")
    efail = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = int(lib.wmf_explain_workspace_bytes(n, c["f"], T))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wmf_explain_rows(_ptr(bufs["Y"]), c["m"], c["f"], c["ld"], c["bias"], _ptr(bufs["W"]), _ptr(ip), _ptr(bufs["indices"]),
                                    _ptr(bufs["values"]), n, _ptr(tg), T, _ptr(contrib), _ptr(total), _ptr(efail), _ptr(ws), need, _stream()))
    torch.cuda.synchronize()
    total = total.cpu().numpy().reshape(n, T).astype(np.float64)
    assert int(efail[0]) == 0
    Yt, beta = ref.tilde(c["Y"][:, :c["f"]], c["bias"])
    worst = 0.0
    for u in range(n):
        lo, hi = int(c["indptr"][u]), int(c["indptr"][u + 1])
        for t, i in enumerate(ce["targets"][u]):
            if i < 0:
                continue
            score = Yt[i] @ X[u, :c["f"]].astype(np.float64) + beta[i]
            if hi == lo:
                assert score == total[u, t] == beta[i]
                continue
            M = max(np.abs(Yt[i]).sum() * np.abs(c["ref"][u]).max(), (hi - lo) * np.abs(ce["ref"][lo:hi, t]).max())
            tol = (c["gate"][u] + ce["gate"][u, t]) * M
            worst = max(worst, abs(score - total[u, t]) / tol)
            assert abs(score - total[u, t]) <= tol, (name, u, t, score, total[u, t], tol)
    print(f"{name}: |y~_i . x_u + beta_i - out_total|, worst difference / tolerance {worst:.3f}")
    record_error("foldin_rows", **{name + "_score_vs_explain_total_over_tol": worst})


def _indefinite_case(bad_value, without_row=False):
    """Unit vectors as items and the identity as W_white: whitened items have norm exactly 1, so the entry (item 3, bad_value)
    makes row 1's I + E_u = diag(.., 1 + bad_value, ..).  ld = f + 4: the rows have padding.  without_row: rows 0 and 2 only."""
    f, m, ld = 8, 8, 12
    rng = np.random.default_rng(3)
    Yf = ref.padded(np.eye(m, f, dtype=np.float32), ld)
    indptr = np.array([0, 3, 5, 9], dtype=np.int64)
    indices = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int32)
    values = rng.uniform(1, 5, 9).astype(np.float32)
    values[3] = bad_value
    if without_row:
        keep = np.r_[0:3, 5:9]
        indptr, indices, values = np.array([0, 3, 7], dtype=np.int64), indices[keep], values[keep]
    return dict(name="indefinite", f=f, ld=ld, bias=0, lam=0.0, m=m, Y=Yf, W32=ref.padded(np.eye(f, dtype=np.float32), ld), indptr=indptr,
                indices=indices, values=values)


def test_an_indefinite_row_is_reported_and_its_neighbours_are_untouched():
    good, fail = _foldin(_indefinite_case(2.0))
    assert fail == 0 and np.isfinite(good).all()
    assert abs(good[1, 3] - 1.0) <= 4 * 2.0 ** -23 and good[1, 4] > 0                 # (w + 1) / (1 + w) = 3 / 3 on axis 3
    without, fail = _foldin(_indefinite_case(2.0, without_row=True))
    assert fail == 0
    for bad_value in (-3.0, -2.0, -1.0):           # pivots 1 - 3 = -2, exactly -1, and exactly 0: each a failure
        X, fail = _foldin(_indefinite_case(bad_value))
        assert fail == 1, bad_value
        assert np.isnan(X[1, :8]).all() and (_bits(X[1, 8:]) == 0).all()
        for u, v in ((0, 0), (2, 1)):
            assert np.array_equal(_bits(X[u]), _bits(good[u])) and np.array_equal(_bits(X[u]), _bits(without[v]))


def test_argument_errors_return_before_any_launch():
    _lib, lib, _ptr, _stream = _api()
    c = ref.case("width_f5_b0_x4")
    need = int(lib.wmf_foldin_workspace_bytes(3, 5))
    assert need >= 1
    bad = [dict(f=0), dict(f=261), dict(ld=4), dict(ld=c["ld"] + 2), dict(m=0), dict(m=1 << 31), dict(n=-1), dict(n=1 << 31),
           dict(ws_bytes=need - 1)]
    bad += [{k: None} for k in ("Y", "W", "indptr", "indices", "values", "X", "fail", "ws")]
    for override in bad:
        X, fail = _foldin(c, expect=_lib.WMF_EINVAL, **override)
        assert (X == SENTINEL).all() and fail == 0, override
    X, fail = _foldin(c, n=0)                                        # no rows: a no-op
    assert (X == SENTINEL).all() and fail == 0
