#!/usr/bin/env python3
"""Times wmf_foldin_rows at the serving shape (profiles/r18_foldin.json): a batch of histories against a catalogue of cfg3's model
shape, folded in three ways on the same box in the same run --
  foldin          one wmf_foldin_rows call, alone and followed by the catalogue scan (wmf_recommend_topn, the histories excluded);
  existing_route  what recompute_factors[_bias] does for the same rows: wmf_row_transform of the WHOLE catalogue, wmf_plan_create,
                  wmf_solve_rows_ex and the un-whitening pass, in the layout the engine chooses;
  torch_float64   torch on the device in float64: the assembled A_u and b of every row, batched linalg.solve.
HIP events around each route, alternating repetitions after a warm-up, median and spread; the answers are compared on the spot.
The Gramian and its factorisation are outside every clock, as WMF.fold_in caches them.

    python tools/foldin_lab.py --out profiles/r18_foldin.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recmodel_amd import _lib  # noqa: E402
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


def summary(runs):
    return {"median_s": float(np.median(runs)), "spread_s": float(max(runs) - min(runs)), "runs_s": [float(x) for x in runs]}


def row_error(x, ref):
    """[rows]: max_a |x - ref| / max_a |ref|."""
    return ((x.to(torch.float64) - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_(min=1e-30))


def shape(lib, n_rows, n_items, k, bias, mean_degree, topn, lam, reps, seed, solve_batch):
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
    # distinct, ascending items within a row: the histories are the scan's seen lists as well
    keys = torch.rand(n_rows, n_items if n_items <= 4096 else 4096, device="cuda", generator=gen)
    dmax = int(deg.max())
    assert dmax <= keys.shape[1]
    stride = n_items // keys.shape[1]
    picks = (torch.argsort(keys, dim=1)[:, :dmax] * stride + torch.randint(0, stride, (n_rows, dmax), device="cuda", generator=gen))
    picks = torch.where(torch.arange(dmax, device="cuda")[None, :] < deg[:, None], picks, torch.full_like(picks, n_items))
    picks = torch.sort(picks, dim=1).values
    indices = picks[picks < n_items].to(torch.int32)
    assert indices.numel() == nnz
    counts = 2.0 + torch.floor(torch.log2(1.0 / (1.0 - torch.rand(nnz, device="cuda", generator=gen)).clamp_(min=1e-12)))
    values = (10 * torch.log1p(counts)).to(torch.float32)

    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    G = torch.empty(f * f, dtype=torch.float64, device="cuda")
    W_white, W_unwhite = (torch.zeros(f, ld, dtype=torch.float32, device="cuda") for _ in range(2))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_gram(_ptr(Y), n_items, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
    _lib.check(lib.wmf_factorize(_ptr(G), f, ld, lam, _ptr(W_white), _ptr(W_unwhite), _ptr(info), _ptr(ws), _stream()))
    assert int(info[0]) == 0

    # ---- wmf_foldin_rows, and the scan behind it
    X = torch.empty(n_rows, ld, dtype=torch.float32, device="cuda")
    fail = torch.zeros(4, dtype=torch.int32, device="cuda")
    fws_bytes = int(lib.wmf_foldin_workspace_bytes(n_rows, f))
    fws = torch.empty(fws_bytes, dtype=torch.uint8, device="cuda")
    ids = torch.arange(n_rows, dtype=torch.int32, device="cuda")
    top_items = torch.empty(n_rows, topn, dtype=torch.int32, device="cuda")
    top_scores = torch.empty(n_rows, topn, dtype=torch.float32, device="cuda")
    sws_bytes = int(lib.wmf_recommend_workspace_bytes(n_rows, topn, 0))
    sws = torch.empty(sws_bytes, dtype=torch.uint8, device="cuda")

    def foldin():
        _lib.check(lib.wmf_foldin_rows(_ptr(Y), n_items, f, ld, bias, _ptr(W_white), _ptr(indptr), _ptr(indices), _ptr(values), n_rows,
                                       _ptr(X), _ptr(fail), _ptr(fws), fws_bytes, _stream()))

    def foldin_and_scan():
        foldin()
        _lib.check(lib.wmf_recommend_topn(_ptr(X), _ptr(Y), f, ld, bias, _ptr(ids), n_rows, n_items, _ptr(indptr), _ptr(indices), topn, 0,
                                          _ptr(top_items), _ptr(top_scores), None, _ptr(sws), sws_bytes, _stream()))

    # ---- the existing route: whiten the whole catalogue, plan, solve, un-whiten (the engine's choice of layout)
    ldv = int(lib.wmf_whitened_row_floats(f, ld, bias))
    split = ldv != ld
    rolled = bool(split and bias and lib.wmf_rolled_layout_supported(f, ld))
    white_mode, unwhite_mode, flags = (3, 4, 1) if rolled else (bias, 0, 0)
    X_route = torch.empty(n_rows, ld, dtype=torch.float32, device="cuda")
    indptr_host = np.ascontiguousarray(indptr.cpu().numpy(), dtype=np.int64)

    def existing_route():
        V = torch.zeros(n_items, ldv, dtype=torch.float32, device="cuda")
        bvec = torch.zeros((n_items, 2) if split else (n_items,), dtype=torch.float32, device="cuda") if bias else None
        g = torch.zeros(n_rows, ld, dtype=torch.float32, device="cuda")
        _lib.check(lib.wmf_row_transform(_ptr(Y), n_items, f, ld, _ptr(W_white), white_mode, _ptr(V), _ptr(bvec), _stream()))
        plan = ctypes.c_void_p()
        _lib.check(lib.wmf_plan_create(indptr_host.ctypes.data_as(ctypes.c_void_p), n_rows, f, bias, ctypes.byref(plan)))
        _lib.check(lib.wmf_solve_rows_ex(plan, _ptr(V), _ptr(bvec), _ptr(indptr), _ptr(indices), _ptr(values), n_rows, f, ld, _ptr(g),
                                         _ptr(fail[1:]), flags, _stream()))
        _lib.check(lib.wmf_row_transform(_ptr(g), n_rows, f, ld, _ptr(W_unwhite), unwhite_mode, _ptr(X_route), None, _stream()))
        torch.cuda.current_stream().synchronize()                  # the plan and the buffers are released with the work done
        lib.wmf_plan_destroy(plan)

    # ---- torch, float64: rows padded to the longest with weight 0 (a padded entry adds nothing to A_u or b)
    col = torch.arange(dmax, device="cuda")[None, :]
    live = col < deg[:, None]
    pos = torch.where(live, indptr[:-1, None] + col, torch.zeros_like(col))
    Gd = G.view(f, f) + lam * torch.eye(f, dtype=torch.float64, device="cuda")
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
        held["x"] = torch.cat([torch.linalg.solve(A[r0:r0 + solve_batch], b[r0:r0 + solve_batch])
                               for r0 in range(0, n_rows, solve_batch)])[:, :, 0]

    foldin_and_scan(), existing_route(), dense()
    torch.cuda.synchronize()
    assert int(fail[0]) == 0 and int(fail[1]) == 0
    ref = held["x"]
    err_foldin, err_route = row_error(X[:, :f], ref), row_error(X_route[:, :f], ref)
    scores = (Y[top_items.long(), :f].to(torch.float64) * ref[:, None, :]).sum(dim=2) if not bias else None
    if bias:
        Yi = Y[top_items.long(), :f].to(torch.float64)
        scores = (Yi[:, :, 1:] * ref[:, None, 1:]).sum(dim=2) + ref[:, None, 0] + Yi[:, :, 0]
    score_err = float((top_scores.to(torch.float64) - scores).abs().max() / scores.abs().max())
    runs = {"foldin": [], "foldin_and_scan": [], "existing_route": [], "torch_float64": []}
    for _ in range(reps):
        runs["foldin"] += timed(foldin, 1)
        runs["foldin_and_scan"] += timed(foldin_and_scan, 1)
        runs["existing_route"] += timed(existing_route, 1)
        runs["torch_float64"] += timed(dense, 1)
    out = {"rows": n_rows, "items": n_items, "k": k, "bias": bias, "mean_entries_per_row": mean_degree, "stored_entries": nnz,
           "longest_row": dmax, "topn": topn, "rows_per_linalg_solve": solve_batch,
           "existing_route_layout": "rolled" if rolled else "split" if split else "plain"}
    out.update({name: summary(r) for name, r in runs.items()})
    out.update({"foldin_worst_row_error_against_torch_float64": float(err_foldin.max()),
                "foldin_median_row_error_against_torch_float64": float(err_foldin.median()),
                "existing_route_worst_row_error_against_torch_float64": float(err_route.max()),
                "existing_route_median_row_error_against_torch_float64": float(err_route.median()),
                "scan_scores_worst_error_against_float64_scores_of_torch_rows": score_err})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--solve-batch", type=int, default=256, help="rows per torch.linalg.solve call")
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0),
           "method": "Per shape, on the same buffers: (foldin) one wmf_foldin_rows call; (foldin_and_scan) the same followed by one "
                     "wmf_recommend_topn over the catalogue with the histories as the seen lists; (existing_route) wmf_row_transform of "
                     "the whole catalogue + wmf_plan_create + wmf_solve_rows_ex + the un-whitening wmf_row_transform, buffers allocated "
                     "inside the clock as recompute_factors[_bias] allocates them; (torch_float64) gather, A_u = G~ + lambda I + U^T "
                     "diag(w) U and b = (w + 1)^T U per row (rows padded to the longest with weight 0), batched torch.linalg.solve "
                     "(rows_per_linalg_solve systems a call).  The Gramian and its factorisation are outside every clock.  HIP events "
                     "around each route on torch's stream (the host work of a route lies between its two events), one warm-up of "
                     "each, then alternating repetitions; median and spread (max - min).  The row error is max_a |x - torch| / "
                     "max_a |torch| per row.",
           "shapes": [shape(lib, args.rows, args.items, args.k, 1, d, args.topn, 0.1, args.reps, 17 + d, args.solve_batch) for d in (10, 100)]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
