#!/usr/bin/env python3
"""Times the posterior calls at the serving shape (profiles/r26_posterior.json): a batch of histories against a catalogue of cfg3's
model shape, on the same box in the same run --
  draws     wmf_posterior_draw_rows at 1 and 16 draws a row against wmf_foldin_rows on the same buffers;
  scores    wmf_posterior_score_rows at 100 and 1000 targets a row;
  torch     the float64 route on the device: the assembled A_u of every row, torch.linalg.cholesky, then cholesky_solve for the mean
            and a triangular solve for 16 draws and for the variances of 100 targets;
  model     WMF.recommend_thompson_for against WMF.recommend_for, and WMF.recommend_ucb_for at pool 100 and 1000 against
            WMF.candidates_for alone, on a model whose items are the same catalogue (host clock around the synchronous calls).
HIP events around each device route, alternating repetitions after a warm-up, median and spread; the answers are compared on the spot.
The Gramian and its factorisation are outside every clock, as the model caches them.

    python tools/posterior_lab.py --out profiles/r26_posterior.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recmodel_amd import WMF, _lib  # noqa: E402
from recmodel_amd.engine import _ptr, _stream  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def host_timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def summary(runs):
    return {"median_s": float(np.median(runs)), "spread_s": float(max(runs) - min(runs)), "runs_s": [float(x) for x in runs]}


def shape(lib, n_rows, n_items, k, bias, mean_degree, lam, reps, seed):
    f = k + bias
    ld = int(lib.wmf_ld_for(f))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    Y = torch.zeros(n_items, ld, dtype=torch.float32, device="cuda")
    Y[:, :f] = torch.rand(n_items, f, device="cuda", generator=gen) / np.sqrt(k)          # item factors; column 0 the bias
    deg = torch.poisson(torch.full((n_rows,), float(mean_degree), device="cuda"), generator=gen).clamp_(min=1).to(torch.int64)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(deg, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    keys = torch.rand(n_rows, min(n_items, 4096), device="cuda", generator=gen)            # distinct, ascending items within a row
    dmax = int(deg.max())
    stride = n_items // keys.shape[1]
    picks = torch.argsort(keys, dim=1)[:, :dmax] * stride + torch.randint(0, stride, (n_rows, dmax), device="cuda", generator=gen)
    picks = torch.where(torch.arange(dmax, device="cuda")[None, :] < deg[:, None], picks, torch.full_like(picks, n_items))
    picks = torch.sort(picks, dim=1).values
    indices = picks[picks < n_items].to(torch.int32)
    assert indices.numel() == nnz
    raw_counts = 2.0 + torch.floor(torch.log2(1.0 / (1.0 - torch.rand(nnz, device="cuda", generator=gen)).clamp_(min=1e-12)))
    values = (10 * torch.log1p(raw_counts)).to(torch.float32)

    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    G = torch.empty(f * f, dtype=torch.float64, device="cuda")
    W_white, W_unwhite = (torch.zeros(f, ld, dtype=torch.float32, device="cuda") for _ in range(2))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_gram(_ptr(Y), n_items, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
    _lib.check(lib.wmf_factorize(_ptr(G), f, ld, lam, _ptr(W_white), _ptr(W_unwhite), _ptr(info), _ptr(ws), _stream()))
    assert int(info[0]) == 0

    head = (_ptr(Y), n_items, f, ld, bias, _ptr(W_white), _ptr(indptr), _ptr(indices), _ptr(values), n_rows)
    fail = torch.zeros(4, dtype=torch.int32, device="cuda")
    pws = torch.empty(256, dtype=torch.uint8, device="cuda")
    X = torch.empty(n_rows, ld, dtype=torch.float32, device="cuda")
    D = {d: torch.empty(n_rows * d, ld, dtype=torch.float32, device="cuda") for d in (1, 16)}
    targets = {t: torch.randint(0, n_items, (n_rows, t), device="cuda", generator=gen).to(torch.int32) for t in (100, 1000)}
    mean = {t: torch.empty(n_rows, t, dtype=torch.float32, device="cuda") for t in targets}
    var = {t: torch.empty(n_rows, t, dtype=torch.float32, device="cuda") for t in targets}

    def foldin():
        _lib.check(lib.wmf_foldin_rows(*head, _ptr(X), _ptr(fail), _ptr(pws), 256, _stream()))

    def draw(d, sigma=1.0):
        _lib.check(lib.wmf_posterior_draw_rows(*head, d, sigma, 5, None, _ptr(D[d]), _ptr(fail), _ptr(pws), 256, _stream()))

    def score(t):
        _lib.check(lib.wmf_posterior_score_rows(*head, _ptr(targets[t]), t, _ptr(mean[t]), _ptr(var[t]), _ptr(fail), _ptr(pws), 256, _stream()))

    # ---- torch, float64: rows padded to the longest with weight 0 (a padded entry adds nothing to A_u or b)
    col = torch.arange(dmax, device="cuda")[None, :]
    live = col < deg[:, None]
    pos = torch.where(live, indptr[:-1, None] + col, torch.zeros_like(col))
    Gd = G.view(f, f) + lam * torch.eye(f, dtype=torch.float64, device="cuda")
    xi = torch.randn(n_rows, f, 16, dtype=torch.float64, device="cuda", generator=gen)
    held = {}

    def dense():
        U = Y[indices[pos].long(), :f].to(torch.float64)                                   # [rows, dmax, f]
        beta = U[:, :, 0].clone() if bias else torch.zeros(n_rows, dmax, dtype=torch.float64, device="cuda")
        if bias:
            U[:, :, 0] = 1.0
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        w = torch.where(live, values[pos].to(torch.float64) - beta, zero)
        A = Gd[None] + U.transpose(1, 2) @ (U * w[:, :, None])
        b = (torch.where(live, w + 1, zero)[:, None, :] @ U).transpose(1, 2)               # [rows, f, 1]
        L = torch.linalg.cholesky(A)
        x = torch.cholesky_solve(b, L)
        held["x"] = x[:, :, 0]
        held["draws"] = x + torch.linalg.solve_triangular(L.transpose(1, 2), xi, upper=True)          # x + L^-T xi: covariance A^-1
        Yi = Y[targets[100].long(), :f].to(torch.float64)                                  # [rows, 100, f]
        if bias:
            Yi[:, :, 0] = 1.0
        Z = torch.linalg.solve_triangular(L, Yi.transpose(1, 2), upper=False)              # [rows, f, 100]
        held["var"] = (Z * Z).sum(dim=1)

    foldin(), draw(1), draw(16), score(100), score(1000), dense()
    draw(1, 0.0)
    torch.cuda.synchronize()
    assert int(fail[0]) == 0
    identical = bool(torch.equal(D[1].view(torch.int32), X.view(torch.int32)))
    draw(1)
    Yi = Y[targets[100].long(), :f].to(torch.float64)
    beta_i = Yi[:, :, 0].clone() if bias else torch.zeros(n_rows, 100, dtype=torch.float64, device="cuda")
    if bias:
        Yi[:, :, 0] = 1.0
    err_mean = float((mean[100].to(torch.float64) - ((Yi * held["x"][:, None, :]).sum(dim=2) + beta_i)).abs().max())
    err_var = float(((var[100].to(torch.float64) - held["var"]).abs() / held["var"]).max())
    runs = {"foldin": [], "draw_1": [], "draw_16": [], "score_100": [], "score_1000": [], "torch_float64": []}
    for _ in range(reps):
        runs["foldin"] += timed(foldin, 1)
        runs["draw_1"] += timed(lambda: draw(1), 1)
        runs["draw_16"] += timed(lambda: draw(16), 1)
        runs["score_100"] += timed(lambda: score(100), 1)
        runs["score_1000"] += timed(lambda: score(1000), 1)
        runs["torch_float64"] += timed(dense, 1)
    out = {"rows": n_rows, "items": n_items, "k": k, "bias": bias, "mean_entries_per_row": mean_degree, "stored_entries": nnz, "longest_row": dmax}
    out.update({name: summary(r) for name, r in runs.items()})
    out.update({"draw_at_sigma_0_is_foldin_bit_for_bit": identical, "var_100_worst_relative_error_against_torch_float64": err_var,
                "mean_100_worst_absolute_error_against_torch_float64": err_mean,
                "torch_float64_computes": "A_u, cholesky, cholesky_solve (the mean), 16 draws, the variances of 100 targets"})

    # ---- the model calls: the same catalogue and histories through WMF
    m = WMF(num_items=n_items, num_users=1, dim=k, gamma=lam, weighted=True, bias=bool(bias))
    m.items = Y[:, :f].cpu().numpy()
    m.users = np.zeros((1, f), dtype=np.float32)
    m.items.flags.writeable = m.users.flags.writeable = False                              # (frozen: the device copies are kept)
    rows = sp.csr_matrix((raw_counts.cpu().numpy().astype(np.float64), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(n_rows, n_items))
    calls = {"recommend_for": lambda: m.recommend_for(rows, 10),
             "recommend_thompson_for": lambda: m.recommend_thompson_for(rows, 10, sigma=1.0, seed=3),
             "candidates_for_100": lambda: m.candidates_for(rows, 100, return_scores=True),
             "recommend_ucb_for_pool_100": lambda: m.recommend_ucb_for(rows, 10, pool=100, c=1.0, return_scores=True),
             "candidates_for_1000": lambda: m.candidates_for(rows, 1000, return_scores=True),
             "recommend_ucb_for_pool_1000": lambda: m.recommend_ucb_for(rows, 10, pool=1000, c=1.0, return_scores=True)}
    for fn in calls.values():
        fn()
    model_runs = {name: [] for name in calls}
    for _ in range(max(3, reps // 2)):
        for name, fn in calls.items():
            model_runs[name].append(host_timed(fn))
    out["model_calls_host_clock"] = {name: summary(r) for name, r in model_runs.items()}
    out["ucb_at_c_0_is_recommend_for"] = bool(np.array_equal(m.recommend_ucb_for(rows, 10, pool=100, c=0), m.recommend_for(rows, 10)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--errors", default=None, help="a parity_errors.json of the GPU tests: its posterior figures are copied in")
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0),
           "method": "Per shape, on the same buffers: wmf_foldin_rows; wmf_posterior_draw_rows at 1 and 16 draws a row (sigma 1); "
                     "wmf_posterior_score_rows at 100 and 1000 random targets a row, both outputs; (torch_float64) gather, A_u = G~ + "
                     "lambda I + U^T diag(w) U per row (rows padded to the longest with weight 0), torch.linalg.cholesky, "
                     "cholesky_solve for the mean, solve_triangular for 16 draws and for the variances of the 100 targets.  The Gramian "
                     "and its factorisation are outside every clock.  HIP events around each route on torch's stream, one warm-up of "
                     "each, then alternating repetitions; median and spread (max - min).  model_calls_host_clock: the WMF methods on "
                     "the same catalogue and histories, host clock between two device synchronisations (uploads, the scans and the "
                     "copy back included), alternating.",
           "shapes": [shape(lib, args.rows, args.items, args.k, 1, d, 0.1, args.reps, 17 + d) for d in (10, 100)]}
    if args.errors and os.path.exists(args.errors):
        got = json.load(open(args.errors)).get("posterior", {})
        mult = {kind: max(v for name, v in got.items() if name.endswith(f"_{kind}_multiple")) for kind in ("draw", "var", "mean")}
        out["gates_measured_by_the_gpu_tests"] = {
            "xi_worst_error_in_units_of_2^-23_max(1,|xi|)": got.get("xi_error_units"),
            "worst_(error - 8 ulps) / restated_error (gate: 4)": mult,
            "orthogonal_catalogue_ulp": {name: v for name, v in got.items() if name.startswith("orthogonal_")},
            "covariance_statistic (gate 37.7)": {name: v for name, v in got.items() if name.startswith("covariance_statistic")}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
