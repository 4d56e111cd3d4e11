"""wmf_explain_rows through the C ABI: every contribution within its gate of the float64 definition (tests/explain_ref.py: the
gate of a (row, target) pair is 4 x the error of the float32 restatement on that pair + 8 ulps), the totals bit for bit the
documented sum, at every width and layout of the serving tests, every row-length edge, target count and input family; the
exactly orthogonal catalogue against fractions.Fraction; determinism, independence of rows and of target columns, sentinels,
the failure report and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref as ref
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


def _explain(c, first=0, count=None, cols=None, expect=0, **override):
    """Rows [first, first + count) of case c through an indptr window, target columns ``cols``.  Returns (contrib [nnz, T] with
    SENTINEL wherever the call may not write, total [count, T], fail count).  Guards around both outputs, the failure counter
    and the workspace are checked here."""
    _lib, lib, _ptr, _stream = _api()
    n_all = len(c["indptr"]) - 1
    count = n_all - first if count is None else count
    targets = np.ascontiguousarray(c["targets"][first:first + count] if cols is None else c["targets"][first:first + count][:, cols])
    T = targets.shape[1]
    nnz = len(c["indices"])
    Yd, Wd = _dev(c["Y"]), _dev(c["W32"])
    # (one spare element each: never empty)
    ip, ix = _dev(c["indptr"][first:first + count + 1], np.int64), _dev(np.append(c["indices"], 0), np.int32)
    vl, tg = _dev(np.append(c["values"], 0), np.float32), _dev(np.append(targets.reshape(-1), 0), np.int32)
    contrib = torch.full((nnz * T + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    total = torch.full((count * T + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    fail = torch.tensor([-7, 0, -7], dtype=torch.int32, device="cuda")
    need = int(lib.wmf_explain_workspace_bytes(count, c["f"], T))
    ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    args = dict(Y=_ptr(Yd), m=c["m"], f=c["f"], ld=c["ld"], bias=c["bias"], W=_ptr(Wd), indptr=_ptr(ip), indices=_ptr(ix), values=_ptr(vl),
                n=count, targets=_ptr(tg), T=T, contrib=ctypes.c_void_p(contrib.data_ptr() + 4 * GUARD),
                total=ctypes.c_void_p(total.data_ptr() + 4 * GUARD), fail=ctypes.c_void_p(fail.data_ptr() + 4), ws=_ptr(ws), ws_bytes=need)
    args.update(override)
    rc = lib.wmf_explain_rows(args["Y"], args["m"], args["f"], args["ld"], args["bias"], args["W"], args["indptr"], args["indices"],
                              args["values"], args["n"], args["targets"], args["T"], args["contrib"], args["total"], args["fail"],
                              args["ws"], args["ws_bytes"], _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.wmf_last_error())
    ch, th, fh = contrib.cpu().numpy(), total.cpu().numpy(), fail.cpu().numpy()
    assert (ch[:GUARD] == SENTINEL).all() and (ch[-GUARD:] == SENTINEL).all(), "out_contrib guards"
    assert (th[:GUARD] == SENTINEL).all() and (th[-GUARD:] == SENTINEL).all(), "out_total guards"
    assert fh[0] == -7 and fh[2] == -7, "fail_count guards"
    assert (ws.cpu().numpy() == 0x5A).all(), "the workspace is reserved, not written"
    return ch[GUARD:-GUARD].reshape(nnz, T), th[GUARD:-GUARD].reshape(count, T), int(fh[1])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_against_reference(c, contrib, total, first=0):
    """Gates, the totals' identity, -1 slots, every element written; returns the pair errors."""
    indptr, tg = c["indptr"], c["targets"]
    n = total.shape[0]
    lo, hi = int(indptr[first]), int(indptr[first + n])
    assert (contrib[:lo] == SENTINEL).all() and (contrib[hi:] == SENTINEL).all(), "entries outside the window were written"
    inside = contrib[lo:hi]
    assert not (inside == SENTINEL).any() and not (total == SENTINEL).any(), "an output element was not written"
    assert np.isfinite(inside).all() and np.isfinite(total).all()
    win = indptr[first:first + n + 1] - lo
    err = ref.pair_errors(inside, c["ref"][lo:hi], win)
    gate = c["gate"][first:first + n]
    live = tg[first:first + n] >= 0
    bad = live & (err > gate)
    assert not bad.any(), (c["name"], [(int(u) + first, int(t), float(err[u, t]), float(gate[u, t])) for u, t in zip(*np.nonzero(bad))][:5])
    for u, t in zip(*np.nonzero(~live)):
        assert (inside[win[u]:win[u + 1], t] == 0).all() and total[u, t] == 0, "a -1 slot writes zeros"
    want = ref.totals_in_order(inside, c["Y"], c["bias"], win, tg[first:first + n])
    assert np.array_equal(_bits(total), _bits(want)), "out_total is not the documented sum of out_contrib"
    return np.where(live, err, 0.0)


@pytest.mark.parametrize("name", ref.case_names())
def test_contributions(name):
    c = ref.case(name)
    contrib, total, fail = _explain(c)
    assert fail == 0
    err = _check_against_reference(c, contrib, total)
    T = c["targets"].shape[1]
    if T >= 4:                                              # the same item twice in one row: identical bits in both columns
        assert np.array_equal(c["targets"][:, 0], c["targets"][:, T - 1])
        assert np.array_equal(_bits(contrib[:, 0]), _bits(contrib[:, T - 1])) and np.array_equal(_bits(total[:, 0]), _bits(total[:, T - 1]))
    u, t = np.unravel_index(err.argmax(), err.shape)
    record_error("explain_rows", **{name: err.max(), name + "_restated": c["restated_err"].max(),
                                    name + "_worst_row_degree": int(c["indptr"][u + 1] - c["indptr"][u])})


@pytest.mark.parametrize("name", ["width_f65_b1_x0", "width_f260_b0_x12", "width_f5_b0_x4"])
def test_indptr_window_and_row_counts(name):
    """A window starting at row 2, three rows, one row: the bits of the full launch, and nothing outside the window is written."""
    c = ref.case(name)
    full, full_total, _ = _explain(c)
    for first, count in ((2, None), (5, 3), (9, 1), (4, 1)):
        contrib, total, fail = _explain(c, first, count)
        n = total.shape[0]
        lo, hi = int(c["indptr"][first]), int(c["indptr"][first + n])
        assert fail == 0
        assert (contrib[:lo] == SENTINEL).all() and (contrib[hi:] == SENTINEL).all()
        assert np.array_equal(_bits(contrib[lo:hi]), _bits(full[lo:hi])) and np.array_equal(_bits(total), _bits(full_total[first:first + n]))
    _check_against_reference(c, *_explain(c, 2)[:2], first=2)


def test_two_runs_and_another_position_give_the_same_bits():
    c = ref.case("width_f129_b1_x0")
    a, at, _ = _explain(c)
    b, bt, _ = _explain(c)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(at), _bits(bt))
    # rows 10 and 3 of the case as rows 0 and 1 of another CSR
    ip = c["indptr"]
    rows = (10, 3)
    moved = dict(c)
    moved["indices"] = np.concatenate([c["indices"][ip[r]:ip[r + 1]] for r in rows])
    moved["values"] = np.concatenate([c["values"][ip[r]:ip[r + 1]] for r in rows])
    moved["indptr"] = np.concatenate([[0], np.cumsum([ip[r + 1] - ip[r] for r in rows])]).astype(np.int64)
    moved["targets"] = c["targets"][list(rows)]
    m, mt, _ = _explain(moved)
    for k, r in enumerate(rows):
        assert np.array_equal(_bits(m[moved["indptr"][k]:moved["indptr"][k + 1]]), _bits(a[ip[r]:ip[r + 1]]))
        assert np.array_equal(_bits(mt[k]), _bits(at[r]))


@pytest.mark.parametrize("name", ["targets_T16", "width_f257_b0_x4"])
def test_a_target_column_does_not_depend_on_the_others(name):
    c = ref.case(name)
    full, full_total, _ = _explain(c)
    T = c["targets"].shape[1]
    for cols in ([0], [T - 1, 1], list(range(T - 1))):
        part, part_total, _ = _explain(c, cols=cols)
        assert np.array_equal(_bits(part), _bits(full[:, cols])) and np.array_equal(_bits(part_total), _bits(full_total[:, cols]))


def test_orthogonal_catalogue_against_fractions():
    """Items are scaled unit vectors: contributions between different axes are exactly 0.0, the others within 2 x the worst ulp
    error of the float32 restatement against the closed form in exact rational arithmetic."""
    c, exact = ref.orthogonal_case()
    bound, measured = ref.orthogonal_ulp_bound()
    contrib, total, fail = _explain(c)
    assert fail == 0
    worst = 0.0
    for u in range(len(c["indptr"]) - 1):
        for e in range(int(c["indptr"][u]), int(c["indptr"][u + 1])):
            for t, i in enumerate(c["targets"][u]):
                if (e, t) in exact:
                    worst = max(worst, ref.ulp_error(contrib[e, t], exact[(e, t)]))
                else:
                    assert c["axis"][i] != c["axis"][c["indices"][e]] and contrib[e, t] == 0.0
    print(f"orthogonal catalogue: device {worst:.3f} ulp, restatement {measured:.3f} ulp, bound {bound:.3f} ulp")
    record_error("explain_rows", orthogonal_ulp=worst, orthogonal_ulp_restated=measured)
    assert worst <= bound


def _indefinite_case(bad_value):
    """Unit vectors as items and the identity as W_white: whitened items have norm exactly 1, so the entry (item 3, bad_value)
    makes row 1's I + E_u = diag(.., 1 + bad_value, ..)."""
    f, m = 8, 8
    rng = np.random.default_rng(3)
    Yf = np.eye(m, f, dtype=np.float32)
    indptr = np.array([0, 3, 5, 9], dtype=np.int64)
    indices = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int32)
    values = rng.uniform(1, 5, 9).astype(np.float32)
    values[3] = bad_value
    targets = np.array([[0, 5, -1], [3, 4, -1], [7, 0, 2]], dtype=np.int32)
    return dict(name="indefinite", f=f, ld=f, bias=0, lam=0.0, m=m, Y=Yf, W32=np.eye(f, dtype=np.float32), indptr=indptr, indices=indices,
                values=values, targets=targets)


def test_an_indefinite_row_is_reported_and_its_neighbours_are_untouched():
    good, good_total, fail = _explain(_indefinite_case(2.0))
    assert fail == 0 and np.isfinite(good).all()
    bad, bad_total, fail = _explain(_indefinite_case(-3.0))          # effective weight -3: the pivot is 1 - 3 = -2
    assert fail == 1
    exact, exact_total, fail0 = _explain(_indefinite_case(-2.0))     # effective weight -2 on a unit direction: the pivot is -1
    assert fail0 == 1
    for c, t in ((bad, bad_total), (exact, exact_total)):
        assert np.isnan(c[3:5, :2]).all() and np.isnan(t[1, :2]).all()
        assert (c[3:5, 2] == 0).all() and t[1, 2] == 0               # the -1 slot of the failed row
        for rows, u in ((slice(0, 3), 0), (slice(5, 9), 2)):
            assert np.array_equal(_bits(c[rows]), _bits(good[rows])) and np.array_equal(_bits(t[u]), _bits(good_total[u]))
    zero_pivot, _, fail1 = _explain(_indefinite_case(-1.0))          # a pivot of exactly 0 is a failure too
    assert fail1 == 1 and np.isnan(zero_pivot[3:5, :2]).all()


def test_argument_errors_return_before_any_launch():
    _lib, lib, _ptr, _stream = _api()
    c = ref.case("width_f5_b0_x4")
    T = c["targets"].shape[1]
    assert lib.wmf_explain_workspace_bytes(3, 5, T) >= 1
    bad = [dict(f=0), dict(f=261), dict(ld=4), dict(ld=c["ld"] + 2), dict(m=0), dict(n=-1), dict(T=0), dict(T=ref.MAX_TARGETS + 1),
           dict(ws_bytes=int(lib.wmf_explain_workspace_bytes(3, 5, T)) - 1)]
    bad += [{k: None} for k in ("Y", "W", "indptr", "indices", "values", "targets", "contrib", "total", "fail", "ws")]
    for override in bad:
        contrib, total, fail = _explain(c, expect=_lib.WMF_EINVAL, **override)
        assert (contrib == SENTINEL).all() and (total == SENTINEL).all() and fail == 0, override
    contrib, total, fail = _explain(c, n=0)                          # no rows: a no-op
    assert (contrib == SENTINEL).all() and (total == SENTINEL).all() and fail == 0
