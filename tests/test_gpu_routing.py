"""Which kernels a half step launches, and how often, pinned per width and layout.

One small matrix holds a row of every kind the launch code tells apart: 3 entries (two rows per wave), 12 and 24 (the two low
bins), 40 and 100 (candidates of the matrix-free iteration), 600 (elimination kernels), 4500 (above WMF_HEAVY_T: segments,
combine, eliminate) and a 40-entry row with one negative weight (bounced to the pivoted kernel).  A half step over it, with the
library's per-kernel table switched on, gives {kernel name: launches}; launch counts are decided on the host, so they are
deterministic, and ROUTES below is what the library launched before its launch code was rewritten around RowArgs / the
block-count dispatcher / the bin schedule (csrc/wmf_internal.h).  Every solved row is compared with oracle.solve_row as well, at
the stated tolerance of its width (test_gpu_parity.py), so that a routing that launches the right names on wrong data fails.

`python tests/test_gpu_routing.py` prints the dictionary of the library it runs against."""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import record_error
from oracle import wmf_oracle as orc

pytestmark = pytest.mark.gpu

M_FIXED = 6000
DEGREES = [3, 3, 12, 12, 24, 24, 40, 40, 100, 100, 600, 600, 4500, 4500, 40]
NEGATIVE_ROW = len(DEGREES) - 1
HALF_FRO, HALF_ROW = 5e-5, 5e-4            # test_gpu_parity.py: f <= 144
WIDE_FRO, WIDE_ROW = 1.5e-4, 1e-3          # f > 144
F64_ROW = 1e-10                            # every float64 test

# (k, bias, rolled): rolled is the engine's default where the library supports it (k = 128 with biases); False there is WMF_ROLLED=0
CASES = [(16, 0, None), (50, 0, None), (64, 0, None), (64, 1, None), (100, 0, None), (128, 0, None), (128, 1, True), (128, 1, False),
         (144, 0, None), (160, 0, None), (208, 1, None), (256, 0, None), (256, 1, None), (260, 0, None)]
# (260, 0): the widest factors the library takes (WMF_MAX_F), and one of the three (258 .. 260) that reach the eight-wave kernel of wmf_wide.hip;
# k = 272 has no plan (wmf_plan_create: "f=272 unsupported"), before and after the rewrite, so it is not a case
F64_WIDTHS = [16, 64, 128, 256]

ROUTES = {
    'k16_bias0': {
        'combine_segments_kernel': 1,
        'factorize64m_kernel': 1,
        'gram_kernel<1, 1>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directw_kernel<1, 0, false>': 1,
        'solve_directw_kernel<1, 1, false>': 1,
        'solve_directw_kernel<1, 2, false>': 1,
        'solve_general_kernel<1>': 1,
        'solve_low_kernel<1, 1, false, false>': 1,
        'solve_low_kernel<1, 2, true, false>': 1,
        'solve_pair_kernel<1, false>': 1,
        'transform_kernel<1, true, 0, 1>': 2,
    },
    'k50_bias0': {
        'combine_segments_kernel': 1,
        'factorize64m_kernel': 1,
        'gram_kernel<4, 1>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directw_kernel<4, 0, false>': 1,
        'solve_directw_kernel<4, 1, false>': 1,
        'solve_directw_kernel<4, 2, false>': 1,
        'solve_general_kernel<4>': 1,
        'solve_low_kernel<4, 1, false, false>': 1,
        'solve_low_kernel<4, 2, true, false>': 1,
        'solve_pair_kernel<4, false>': 1,
        'transform_kernel<4, true, 0, 4>': 2,
    },
    'k64_bias0': {
        'combine_segments_kernel': 1,
        'factorize64m_kernel': 1,
        'gram_kernel<4, 1>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directl_kernel<4, false, true, 16, 0>': 1,
        'solve_directw_kernel<4, 1, false>': 1,
        'solve_directw_kernel<4, 2, false>': 1,
        'solve_general_kernel<4>': 1,
        'solve_low_kernel<4, 1, false, true>': 1,
        'solve_low_kernel<4, 2, true, true>': 1,
        'solve_pair_kernel<4, true>': 1,
        'transform_kernel<4, true, 0, 4>': 2,
    },
    'k64_bias1': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram_kernel<5, 1>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directl_kernel<4, true, true, 16, 0>': 1,
        'solve_directw_kernel<4, 1, true>': 1,
        'solve_directw_kernel<4, 2, true>': 1,
        'solve_general_kernel<5>': 1,
        'solve_low_kernel<5, 1, false, true>': 1,
        'solve_low_kernel<5, 2, true, true>': 1,
        'solve_pair_kernel<5, true>': 1,
        'transform_kernel<5, true, 0, 5>': 2,
    },
    'k100_bias0': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram6_kernel<7>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directw_kernel<7, 0, false>': 1,
        'solve_directw_kernel<7, 0, false> [bounced]': 1,
        'solve_directw_kernel<7, 1, false>': 1,
        'solve_directw_kernel<7, 2, false>': 1,
        'solve_general_kernel<7>': 1,
        'solve_iter_kernel<4, 8, 9, false, false, 3, false, false>': 1,
        'solve_low_kernel<7, 1, false, false>': 1,
        'solve_low_kernel<7, 2, true, false>': 1,
        'solve_pair_kernel<7, false>': 1,
        'transform6_kernel<7>': 2,
    },
    'k128_bias0': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram6_kernel<8>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directl_kernel<8, false, true, 8, 0>': 1,
        'solve_directl_kernel<8, false, true, 8, 0> [bounced]': 1,
        'solve_directl_kernel<8, false, true, 8, 1>': 1,
        'solve_directw_kernel<8, 2, false>': 1,
        'solve_general_kernel<8>': 1,
        'solve_iter_kernel<2, 8, 16, false, true, 2, false, false>': 1,
        'solve_iter_kernel<4, 8, 8, false, true, 2, true, false>': 1,
        'solve_low_kernel<8, 1, false, true>': 1,
        'solve_low_kernel<8, 2, true, true>': 1,
        'solve_pair_kernel<8, true>': 1,
        'transform6_kernel<8>': 2,
    },
    'k128_bias1_rolled': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram6_kernel<9>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directl_kernel<8, true, true, 8, 0>': 1,
        'solve_directl_kernel<8, true, true, 8, 0> [bounced]': 1,
        'solve_directl_kernel<8, true, true, 8, 1>': 1,
        'solve_directw_kernel<8, 2, true>': 1,
        'solve_general_kernel<9>': 1,
        'solve_iter_kernel<2, 8, 16, true, true, 2, false, true>': 1,
        'solve_iter_kernel<4, 8, 8, true, true, 2, true, true>': 1,
        'solve_low_kernel<9, 1, false, true>': 1,
        'solve_low_kernel<9, 2, true, true>': 1,
        'solve_pair_kernel<9, true>': 1,
        'transform6_kernel<9>': 2,
    },
    'k128_bias1_plain': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram6_kernel<9>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directl_kernel<8, true, true, 8, 0>': 1,
        'solve_directl_kernel<8, true, true, 8, 0> [bounced]': 1,
        'solve_directl_kernel<8, true, true, 8, 1>': 1,
        'solve_directw_kernel<8, 2, true>': 1,
        'solve_general_kernel<9>': 1,
        'solve_iter_kernel<2, 8, 16, true, true, 2, false, false>': 1,
        'solve_iter_kernel<4, 8, 8, true, true, 2, true, false>': 1,
        'solve_low_kernel<9, 1, false, true>': 1,
        'solve_low_kernel<9, 2, true, true>': 1,
        'solve_pair_kernel<9, true>': 1,
        'transform6_kernel<9>': 2,
    },
    'k144_bias0': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram6_kernel<9>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_directw_kernel<9, 0, false>': 1,
        'solve_directw_kernel<9, 0, false> [bounced]': 1,
        'solve_directw_kernel<9, 1, false>': 1,
        'solve_directw_kernel<9, 2, false>': 1,
        'solve_general_kernel<9>': 1,
        'solve_iter_kernel<8, 12, 8, false, false, 2, false, false>': 1,
        'solve_low_kernel<9, 1, false, false>': 1,
        'solve_low_kernel<9, 2, true, false>': 1,
        'solve_pair_kernel<9, false>': 1,
        'transform6_kernel<9>': 2,
    },
    'k160_bias0': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram_kernel<10, 4>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_iter_kernel<8, 12, 8, false, false, 2, false, false>': 1,
        'solve_low_kernel<10, 1, false, true>': 1,
        'solve_low_kernel<10, 2, true, true>': 1,
        'solve_pair_kernel<10, true>': 1,
        'solve_rowsplit_kernel<10, false, true, 0>': 1,
        'solve_rowsplit_kernel<10, false, true, 0> [bounced]': 1,
        'solve_rowsplit_kernel<10, false, true, 1>': 1,
        'solve_rowsplit_kernel<10, false, true, 2>': 1,
        'solve_wide_lu_kernel': 1,
        'transform_kernel<10, true, 0, 10>': 2,
    },
    'k208_bias1': {
        'bias_adjust_kernel': 1,
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram_kernel<14, 4>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_iter_kernel<8, 16, 8, false, false, 2, false, false>': 1,
        'solve_low_kernel<14, 1, false, false>': 1,
        'solve_low_kernel<14, 2, true, false>': 1,
        'solve_pair_kernel<14, false>': 1,
        'solve_rowsplit_kernel<13, true, true, 0>': 1,
        'solve_rowsplit_kernel<13, true, true, 0> [bounced]': 1,
        'solve_rowsplit_kernel<13, true, true, 1>': 1,
        'solve_rowsplit_kernel<13, true, true, 2>': 1,
        'solve_wide_lu_kernel': 1,
        'transform_kernel<14, true, 0, 7>': 2,
        'transform_kernel<14, true, 7, 7>': 2,
    },
    'k256_bias0': {
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram_kernel<16, 4>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_iter_kernel<8, 16, 8, false, true, 2, false, false>': 1,
        'solve_low_kernel<16, 1, false, true>': 1,
        'solve_low_kernel<16, 2, true, true>': 1,
        'solve_pair_kernel<16, true>': 1,
        'solve_rowsplit_kernel<16, false, true, 0>': 1,
        'solve_rowsplit_kernel<16, false, true, 0> [bounced]': 1,
        'solve_rowsplit_kernel<16, false, true, 1>': 1,
        'solve_rowsplit_kernel<16, false, true, 2>': 1,
        'solve_wide_lu_kernel': 1,
        'transform_kernel<16, true, 0, 8>': 2,
        'transform_kernel<16, true, 8, 8>': 2,
    },
    'k256_bias1': {
        'bias_adjust_kernel': 1,
        'combine_segments_kernel': 1,
        'factorize_blocked_kernel': 1,
        'gram_kernel<17, 4>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_iter_kernel<8, 20, 6, false, false, 2, false, false>': 1,
        'solve_low_kernel<17, 1, false, true>': 1,
        'solve_low_kernel<17, 2, true, true>': 1,
        'solve_pair_kernel<17, true>': 1,
        'solve_rowsplit_kernel<16, true, true, 0>': 1,
        'solve_rowsplit_kernel<16, true, true, 0> [bounced]': 1,
        'solve_rowsplit_kernel<16, true, true, 1>': 1,
        'solve_rowsplit_kernel<16, true, true, 2>': 1,
        'solve_wide_lu_kernel': 1,
        'transform_kernel<17, true, 0, 6>': 2,
        'transform_kernel<17, true, 12, 5>': 2,
        'transform_kernel<17, true, 6, 6>': 2,
    },
    'k260_bias0': {
        'factorize_blocked_kernel': 1,
        'gram_kernel<17, 4>': 1,
        'gram_reduce1_kernel': 1,
        'gram_reduce2_kernel': 1,
        'solve_iter_kernel<8, 20, 6, false, false, 2, false, false>': 1,
        'solve_low_kernel<17, 1, false, false>': 1,
        'solve_low_kernel<17, 2, true, false>': 1,
        'solve_pair_kernel<17, false>': 1,
        'solve_wide_kernel<17>': 1,
        'solve_wide_kernel<17> [bounced]': 1,
        'solve_wide_lu_kernel': 1,
        'transform_kernel<17, true, 0, 6>': 2,
        'transform_kernel<17, true, 12, 5>': 2,
        'transform_kernel<17, true, 6, 6>': 2,
    },
    'f64_k16': {
        'factor64_kernel<1>': 1,
        'gram64m_kernel<1>': 1,
        'gram64v2_reduce_kernel': 1,
        'rinv64_kernel': 1,
        'solve64_lu_kernel': 1,
        'solve64it_kernel<1, 4, 8>': 1,
        'solve64it_kernel<4, 4, 16>': 1,
        'solve64lr_kernel': 1,
        'solve64v2_kernel<1, 64, 8>': 1,
        'transform64m_kernel<16, 2>': 2,
    },
    'f64_k64': {
        'factor64_kernel<1>': 1,
        'gram64m_kernel<2>': 1,
        'gram64v2_reduce_kernel': 1,
        'rinv64_kernel': 1,
        'solve64_lu_kernel': 1,
        'solve64it_kernel<1, 4, 8>': 1,
        'solve64it_kernel<4, 4, 16>': 1,
        'solve64lr_kernel': 1,
        'solve64v2_kernel<3, 64, 8>': 1,
        'transform64m_kernel<16, 2>': 2,
    },
    'f64_k128': {
        'factor64_kernel<3>': 1,
        'gram64m_kernel<5>': 1,
        'gram64v2_reduce_kernel': 1,
        'rinv64_kernel': 1,
        'solve64_lu_kernel': 1,
        'solve64it_kernel<1, 8, 8>': 1,
        'solve64it_kernel<4, 8, 9>': 1,
        'solve64lr_kernel': 1,
        'solve64v2_kernel<3, 256, 16>': 1,
        'transform64m_kernel<32, 3>': 2,
    },
    'f64_k256': {
        'factor64_kernel<9>': 1,
        'gram64v2_kernel<9>': 1,
        'gram64v2_reduce_kernel': 1,
        'rinv64_kernel': 1,
        'solve64_lu_kernel': 1,
        'solve64lr_kernel': 1,
        'solve64v2_kernel<9, 256, 16>': 1,
        'transform64_kernel<1>': 2,
    },
}


def case_id(k, bias, rolled):
    return f"k{k}_bias{bias}" + ("" if rolled is None else ("_rolled" if rolled else "_plain"))


_MATRIX = []


def matrix():
    """(indptr, indices, weights) of the 15 solved rows, built once."""
    if not _MATRIX:
        rng = np.random.default_rng(2024)
        indptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
        indices = np.concatenate([np.sort(rng.choice(M_FIXED, d, replace=False)) for d in DEGREES]).astype(np.int64)
        w = (10 * np.log(1 + rng.integers(1, 8, indptr[-1]))).astype(np.float32)
        w[indptr[NEGATIVE_ROW] + 7] = -2.0
        _MATRIX.extend((indptr, indices, w))
    return _MATRIX


def fixed_side(k, bias):
    from recmodel_amd import WMF
    Y = WMF(num_items=M_FIXED, num_users=1, dim=k, gamma=0.1, weighted=True, bias=bool(bias), seed=k).items
    if bias:
        Y[:, 0] *= 0.5
    return Y


def launches(lib, run):
    """{kernel name: launches} of run()."""
    from recmodel_amd import _lib
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


def check_rows(got, Y, bias, gate_row, gate_fro, name):
    indptr, indices, w = matrix()
    Yd = Y.astype(np.float64)
    Gy = Yd.copy()
    if bias:
        Gy[:, 0] = 1.0
    G = Gy.T @ Gy + 0.1 * np.eye(Y.shape[1])
    worst, num, den = 0.0, 0.0, 0.0
    for u in range(len(DEGREES)):
        lo, hi = indptr[u], indptr[u + 1]
        idx, ww = indices[lo:hi], w[lo:hi].astype(np.float64)
        if bias:
            ww = ww - Yd[idx, 0]
        want = orc.solve_row(G, Gy[idx], np.arange(hi - lo), ww)
        e, n_ = np.linalg.norm(got[u] - want), np.linalg.norm(want)
        worst = max(worst, e / n_)
        num += e * e
        den += n_ * n_
    fro = float(np.sqrt(num / den))
    record_error(name, worst_row=worst, fro=fro)
    print(f"{name}: worst row {worst:.3e}, fro {fro:.3e}")
    assert worst <= gate_row and fro <= gate_fro, (name, worst, fro)


def route_f32(k, bias, rolled):
    from recmodel_amd import _lib
    from recmodel_amd.engine import AlsEngine
    lib = _lib.load()
    indptr, indices, w = matrix()
    old = os.environ.get("WMF_ROLLED")
    if rolled is False:
        os.environ["WMF_ROLLED"] = "0"
    try:
        eng = AlsEngine(len(DEGREES), M_FIXED, k, bool(bias), 0.1)
    finally:
        if rolled is False:
            if old is None:
                del os.environ["WMF_ROLLED"]
            else:
                os.environ["WMF_ROLLED"] = old
    assert rolled is None or eng.rolled == rolled
    eng.set_interactions(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(w).cuda())
    Y = fixed_side(k, bias)
    eng.set_factors("items", Y)
    table = launches(lib, lambda: eng.half_step("users"))
    eng.check_numerics()
    gate = (HALF_ROW, HALF_FRO) if eng.f <= 144 else (WIDE_ROW, WIDE_FRO)
    check_rows(eng.get_factors("users").astype(np.float64), Y, bias, *gate, name=f"routing[{case_id(k, bias, rolled)}]")
    return table


def route_f64(k):
    from recmodel_amd import _lib
    from recmodel_amd.engine import HipKernels
    lib = _lib.load()
    K = HipKernels()
    indptr, indices, w = matrix()
    n = len(DEGREES)
    dev = torch.device("cuda:0")
    Y = np.random.default_rng(k).random((M_FIXED, k))
    Yd = torch.from_numpy(Y).to(dev)
    ip, ix, wd = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices.astype(np.int32)).to(dev), torch.from_numpy(w.astype(np.float64)).to(dev)
    ws = torch.empty(K.half_step_f64_workspace_bytes(k, M_FIXED, n), dtype=torch.uint8, device=dev)
    fail = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.empty(n, k, dtype=torch.float64, device=dev)
    table = launches(lib, lambda: K.half_step_f64(Yd, M_FIXED, k, False, ip, ix, wd, n, 0.1, out, ws, fail))
    assert int(fail[0]) == 0
    check_rows(out.cpu().numpy(), Y, 0, F64_ROW, F64_ROW, name=f"routing[f64_k{k}]")
    return table


@pytest.mark.parametrize("k,bias,rolled", CASES, ids=[case_id(*c) for c in CASES])
def test_float32_half_step_launches_the_pinned_kernels(k, bias, rolled):
    got = route_f32(k, bias, rolled)
    assert got == ROUTES[case_id(k, bias, rolled)], got


@pytest.mark.parametrize("k", F64_WIDTHS)
def test_float64_half_step_launches_the_pinned_kernels(k):
    got = route_f64(k)
    assert got == ROUTES[f"f64_k{k}"], got


if __name__ == "__main__":
    import pprint
    routes = {case_id(*c): route_f32(*c) for c in CASES}
    routes.update({f"f64_k{k}": route_f64(k) for k in F64_WIDTHS})
    print("ROUTES = " + pprint.pformat(routes, width=150, sort_dicts=True))
