#!/usr/bin/env python3
"""Measure wmf_sample_topn against wmf_recommend_topn_wide on the same device buffers, wmf_log_partition alone, and the route a
caller had to write without them.

Shape: 2048 and 16 rows, a million items, k = 128 + biases (f = 129), Gaussian factors from a seed, 10 seen items per row.  For each
(rows, n, T), in alternating repetitions of one process, each a host clock around work that ends in a device synchronise:
  sample    wmf_sample_topn (n = 10 / 100 / 1000, T = 0 / 1);
  wide      wmf_recommend_topn_wide at topn = n on the same buffers and workspace: what the sampling scan costs is the ratio.
Per rows: wmf_log_partition at T = 1.  Once, at a batch whose score matrix fits (--torch-rows): the torch route -- scores by matmul,
the seen items masked, Gumbel noise from torch's generator, topk.  The kernels' own times come from wmf_profile_*.  Needs a GPU;
writes one JSON file.

    python tools/sample_lab.py --out build/sample_lab.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recmodel_amd import _lib                                      # noqa: E402
from recmodel_amd.engine import _ptr, _stream                      # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def stats(runs):
    return {"median_s": float(np.median(runs)), "spread_s": float(max(runs) - min(runs)), "runs_s": [float(x) for x in runs]}


def kernels(lib, fn):
    """{kernel: seconds} of one call."""
    torch.cuda.synchronize()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.wmf_profile_enable(0)
    table = {name: ms / 1e3 for name, _tag, ms, *_ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[2048, 16])
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--n", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--seen", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=64)
    ap.add_argument("--out", default="build/sample_lab.json")
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    bias, f = 1, args.k + 1
    ld = int(lib.wmf_ld_for(f))
    gen = torch.Generator(device="cuda").manual_seed(25)
    items_t = torch.zeros(args.items, ld, device="cuda")
    items_t[:, :f] = torch.randn(args.items, f, generator=gen, device="cuda")
    most = max(args.rows + [args.torch_rows])
    users_t = torch.zeros(most, ld, device="cuda")
    users_t[:, :f] = torch.randn(most, f, generator=gen, device="cuda")
    uid = torch.arange(most, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(25)
    seen = np.sort(rng.integers(0, args.items, (most, args.seen)), axis=1)
    indptr = torch.from_numpy(np.arange(most + 1, dtype=np.int64) * args.seen).cuda()
    indices = torch.from_numpy(seen.astype(np.int32).ravel()).cuda()
    head = (_ptr(users_t), _ptr(items_t), f, ld, bias, _ptr(uid))
    nofilter = (None, 0, 0, None, None, 0)
    result = {"device": torch.cuda.get_device_name(0), "items": args.items, "k": args.k, "bias": bias, "seen_per_row": args.seen,
              "reps": args.reps, "shapes": [], "log_partition": []}
    for rows in args.rows:
        for n in args.n:
            need = int(lib.wmf_sample_workspace_bytes(rows, n, 0))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            o_items = torch.empty(rows, n, dtype=torch.int32, device="cuda")
            o_scores = torch.empty(rows, n, dtype=torch.float32, device="cuda")
            w_items, w_scores = torch.empty_like(o_items), torch.empty_like(o_scores)

            def wide():
                _lib.check(lib.wmf_recommend_topn_wide(*head, rows, args.items, _ptr(indptr), _ptr(indices), *nofilter, n, 0, _ptr(w_items),
                                                       _ptr(w_scores), None, _ptr(ws), need, _stream()))

            for T in (0.0, 1.0):
                def sample():
                    _lib.check(lib.wmf_sample_topn(*head, rows, args.items, _ptr(indptr), _ptr(indices), *nofilter, n, 0, T, 25, None,
                                                   _ptr(o_items), _ptr(o_scores), None, None, _ptr(ws), need, _stream()))
                wide()
                sample()
                s_runs, w_runs = [], []
                for _ in range(args.reps):                          # alternating
                    s_runs.append(timed(sample))
                    w_runs.append(timed(wide))
                row = {"rows": rows, "n": n, "temperature": T, "workspace_bytes": need, "sample": stats(s_runs), "wide": stats(w_runs),
                       "sample_kernels_s": kernels(lib, sample), "wide_kernels_s": kernels(lib, wide)}
                row["sample_over_wide"] = row["sample"]["median_s"] / row["wide"]["median_s"]
                if T == 0.0:
                    row["same_bits_as_wide"] = bool(torch.equal(o_items, w_items) and torch.equal(o_scores.view(torch.int32), w_scores.view(torch.int32)))
                result["shapes"].append(row)
                print(json.dumps({k: row[k] for k in ("rows", "n", "temperature", "sample_over_wide")}), row["sample"]["median_s"],
                      row["wide"]["median_s"], flush=True)
            del ws
            torch.cuda.empty_cache()
        need = int(lib.wmf_log_partition_workspace_bytes(rows, 0))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        logz = torch.empty(rows, dtype=torch.float32, device="cuda")

        def partition():
            _lib.check(lib.wmf_log_partition(*head, rows, args.items, _ptr(indptr), _ptr(indices), *nofilter, 1.0, 0, _ptr(logz), None, _ptr(ws),
                                             need, _stream()))
        partition()
        row = {"rows": rows, "temperature": 1.0, "workspace_bytes": need, "call": stats([timed(partition) for _ in range(args.reps)]),
               "kernels_s": kernels(lib, partition)}
        if rows <= args.torch_rows:
            S = users_t[:rows, bias:f].double() @ items_t[:, bias:f].double().T + users_t[:rows, :1].double() + items_t[:, 0].double()[None, :]
            S[torch.arange(rows, device="cuda").repeat_interleave(args.seen), indices[:rows * args.seen].long()] = -float("inf")
            row["worst_error_against_float64"] = float((logz.double() - torch.logsumexp(S, dim=1)).abs().max())
            del S
        result["log_partition"].append(row)
        print("log_partition", rows, row["call"]["median_s"], flush=True)
        del ws
        torch.cuda.empty_cache()

    # the torch route: scores, mask, Gumbel noise, topk
    rows = args.torch_rows
    tgen = torch.Generator(device="cuda").manual_seed(1)
    seen_rows = torch.arange(rows, device="cuda").repeat_interleave(args.seen)
    seen_cols = indices[:rows * args.seen].long()
    route = []
    for n in args.n:
        def baseline():
            S = users_t[:rows, bias:f] @ items_t[:, bias:f].T + users_t[:rows, :1] + items_t[:, 0][None, :]
            S[seen_rows, seen_cols] = -float("inf")
            u = torch.rand(S.shape, generator=tgen, device="cuda").clamp_(2.0 ** -24, 1 - 2.0 ** -24)
            return torch.topk(S - torch.log(-torch.log(u)), n, dim=1)
        baseline()
        need = int(lib.wmf_sample_workspace_bytes(rows, n, 0))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        o_items = torch.empty(rows, n, dtype=torch.int32, device="cuda")

        def sample():
            _lib.check(lib.wmf_sample_topn(*head, rows, args.items, _ptr(indptr), _ptr(indices), *nofilter, n, 0, 1.0, 25, None, _ptr(o_items),
                                           None, None, None, _ptr(ws), need, _stream()))
        sample()
        t_runs, s_runs = [], []
        for _ in range(args.reps):
            t_runs.append(timed(baseline))
            s_runs.append(timed(sample))
        route.append({"rows": rows, "n": n, "temperature": 1.0, "score_matrix_bytes": 4 * rows * args.items, "torch": stats(t_runs),
                      "sample": stats(s_runs), "torch_over_sample": float(np.median(t_runs) / np.median(s_runs))})
        print("torch route", n, route[-1]["torch"]["median_s"], route[-1]["sample"]["median_s"], flush=True)
    result["torch_route"] = route
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
