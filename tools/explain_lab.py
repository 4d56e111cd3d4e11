#!/usr/bin/env python3
"""Times wmf_explain_rows at the serving shape (profiles/r17_explain.json): one call for a batch of users x targets against a
catalogue of cfg3's model shape, next to the same numbers computed with torch on the device in float64 -- the assembled A_u of
every row, batched linalg.solve, the second pass as a batched matmul.  HIP events around each path, alternating repetitions
after a warm-up, median and spread; the two answers are compared on the spot.

    python tools/explain_lab.py --out profiles/r17_explain.json
"""
import argparse
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


def shape(lib, n_rows, n_items, k, bias, mean_degree, n_targets, lam, reps, seed, solve_batch):
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
    indices = torch.randint(0, n_items, (nnz,), device="cuda", generator=gen).to(torch.int32)
    counts = 2.0 + torch.floor(torch.log2(1.0 / (1.0 - torch.rand(nnz, device="cuda", generator=gen)).clamp_(min=1e-12)))
    values = (10 * torch.log1p(counts)).to(torch.float32)
    targets = torch.randint(0, n_items, (n_rows, n_targets), device="cuda", generator=gen).to(torch.int32)

    ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
    G = torch.empty(f * f, dtype=torch.float64, device="cuda")
    W_white, W_unwhite = (torch.zeros(f, ld, dtype=torch.float32, device="cuda") for _ in range(2))
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.wmf_gram(_ptr(Y), n_items, f, ld, bias, _ptr(G), _ptr(ws), _stream()))
    _lib.check(lib.wmf_factorize(_ptr(G), f, ld, lam, _ptr(W_white), _ptr(W_unwhite), _ptr(info), _ptr(ws), _stream()))
    assert int(info[0]) == 0

    contrib = torch.empty(nnz, n_targets, dtype=torch.float32, device="cuda")
    total = torch.empty(n_rows, n_targets, dtype=torch.float32, device="cuda")
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    ews_bytes = int(lib.wmf_explain_workspace_bytes(n_rows, f, n_targets))
    ews = torch.empty(ews_bytes, dtype=torch.uint8, device="cuda")

    def device():
        _lib.check(lib.wmf_explain_rows(_ptr(Y), n_items, f, ld, bias, _ptr(W_white), _ptr(indptr), _ptr(indices), _ptr(values), n_rows,
                                        _ptr(targets), n_targets, _ptr(contrib), _ptr(total), _ptr(fail), _ptr(ews), ews_bytes, _stream()))

    # torch, float64: rows padded to the longest with weight 0 (a padded entry adds nothing to A_u)
    dmax = int(deg.max())
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
        w = torch.where(live, values[pos].to(torch.float64) - beta, torch.zeros((), dtype=torch.float64, device="cuda"))
        A = Gd[None] + U.transpose(1, 2) @ (U * w[:, :, None])
        Yi = Y[targets.long(), :f].to(torch.float64)                                       # [rows, targets, f]
        if bias:
            Yi[:, :, 0] = 1.0
        B = Yi.transpose(1, 2)                                                             # [rows, f, targets]
        X = torch.cat([torch.linalg.solve(A[r0:r0 + solve_batch], B[r0:r0 + solve_batch]) for r0 in range(0, n_rows, solve_batch)])
        held["c"] = (w + 1)[:, :, None] * (U @ X)
        held["live"] = live

    device(), dense()
    torch.cuda.synchronize()
    assert int(fail[0]) == 0
    ref = held["c"][held["live"]]                                                          # [nnz, targets], stored order
    scale = torch.zeros(n_rows, n_targets, dtype=torch.float64, device="cuda")
    rows = torch.repeat_interleave(torch.arange(n_rows, device="cuda"), deg)
    scale.index_reduce_(0, rows, ref.abs(), "amax", include_self=True)
    err = torch.zeros_like(scale)
    err.index_reduce_(0, rows, (contrib.to(torch.float64) - ref).abs(), "amax", include_self=True)
    pair = (err / scale.clamp_(min=1e-30))
    runs = {"explain": [], "torch_float64": []}
    for _ in range(reps):
        runs["explain"] += timed(device, 1)
        runs["torch_float64"] += timed(dense, 1)
    return {"rows": n_rows, "targets": n_targets, "items": n_items, "k": k, "bias": bias, "mean_entries_per_row": mean_degree,
            "stored_entries": nnz, "longest_row": dmax, "rows_per_linalg_solve": solve_batch, "explain": summary(runs["explain"]),
            "torch_float64": summary(runs["torch_float64"]),
            "worst_pair_error_against_torch_float64": float(pair.max()), "median_pair_error_against_torch_float64": float(pair.median())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--solve-batch", type=int, default=256, help="rows per torch.linalg.solve call (one call of 2048 systems of 129 x 129 "
                    "failed to allocate its batched-LU workspace)")
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0),
           "method": "One wmf_explain_rows call (C ABI; Gramian and factorisation of the catalogue outside the clock, as WMF.explain caches "
                     "them) next to torch on the device in float64: gather, A_u = G~ + lambda I + U^T diag(w) U per row (rows padded to the "
                     "longest with weight 0), batched torch.linalg.solve for all targets (rows_per_linalg_solve systems a call), the "
                     "second pass as a batched matmul.  HIP events around each path on torch's stream, one warm-up of each, then "
                     "alternating repetitions; median and spread (max - min).  The pair error is max_e |device - torch| / max_e |torch| per (row, target).",
           "shapes": [shape(lib, args.rows, args.items, args.k, 1, d, args.targets, 0.1, args.reps, 17 + d, args.solve_batch) for d in (10, 100)]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
