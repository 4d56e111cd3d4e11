#!/usr/bin/env python3
"""Measure wmf_rerank_mmr against what a caller had to write before it, on the same device buffers.

Shape: 2048 rows, a million items, k = 128 + biases (f = 129), Gaussian factors from a seed.  For each (pool, topn) the candidate
pool is made once by wmf_recommend_topn_wide (its time is reported: the scan the re-rank follows); then, in five alternating
repetitions of one process, each a host clock around work that ends in a device synchronise:
  library   wmf_rerank_mmr on the pool buffers (cosine);
  torch     gather the pool rows (rows x pool x k floats), normalise them, then topn steps of batched product, running max and
            argmax.
Reported: median and spread (max - min) of both, the bytes the kernel's variant reads by its own count (resident: rows x pool x
row, once; streaming: rows x pool x (picks - 1) x row) over its time, which kernel ran (wmf_profile_*), the re-rank as a share of the
scan, and whether the two routes return the same lists.  Needs a GPU; writes one JSON file.

    python tools/mmr_lab.py --out build/mmr_lab.json
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

SHAPES = ((100, 10), (200, 10), (1000, 10), (1000, 50))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def stats(runs):
    return {"median_s": float(np.median(runs)), "spread_s": float(max(runs) - min(runs)), "runs_s": [float(x) for x in runs]}


def torch_mmr(items_t, bias, inv, pool_items, pool_scores, lam, topn):
    """The route without the kernel: gather, normalise, topn steps of product, max and argmax."""
    B, pool = pool_items.shape
    idx = pool_items.long()
    X = items_t[idx][:, :, bias:] * inv[idx][:, :, None]           # [B, pool, ld - bias]: the padding columns are zero
    a = lam * pool_scores
    v = a.clone()
    taken = torch.zeros(B, pool, dtype=torch.bool, device=X.device)
    m = None
    rows = torch.arange(B, device=X.device)
    out = torch.empty(B, topn, dtype=torch.int64, device=X.device)
    for t in range(topn):
        p = torch.where(taken, torch.full_like(v, -float("inf")), v).argmax(dim=1)
        out[:, t] = idx[rows, p]
        taken[rows, p] = True
        if t + 1 < topn:
            s = torch.bmm(X, X[rows, p].unsqueeze(2)).squeeze(2)
            m = s if m is None else torch.maximum(m, s)
            v = a - (1.0 - lam) * m
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="build/mmr_lab.json")
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    bias, f = 1, args.k + 1
    ld = int(lib.wmf_ld_for(f))
    gen = torch.Generator(device="cuda").manual_seed(21)
    items_t = torch.zeros(args.items, ld, device="cuda")
    items_t[:, :f] = torch.randn(args.items, f, generator=gen, device="cuda")
    users_t = torch.zeros(args.rows, ld, device="cuda")
    users_t[:, :f] = torch.randn(args.rows, f, generator=gen, device="cuda")
    uid = torch.arange(args.rows, dtype=torch.int32, device="cuda")
    inv = torch.empty(args.items, device="cuda")
    _lib.check(lib.wmf_row_inv_norms(_ptr(items_t), args.items, f, ld, bias, _ptr(inv), _stream()))
    resident = int(lib.wmf_rerank_mmr_resident_pool(f, ld))
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "items": args.items, "k": args.k, "bias": bias, "lam": args.lam,
              "resident_pool": resident, "row_bytes": 4 * ld, "shapes": []}
    for pool, topn in SHAPES:
        need = int(lib.wmf_recommend_wide_workspace_bytes(args.rows, pool, 0))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        p_items = torch.empty(args.rows, pool, dtype=torch.int32, device="cuda")
        p_scores = torch.empty(args.rows, pool, dtype=torch.float32, device="cuda")
        p_count = torch.empty(args.rows, dtype=torch.int32, device="cuda")
        out_items = torch.empty(args.rows, topn, dtype=torch.int32, device="cuda")

        def scan():
            _lib.check(lib.wmf_recommend_topn_wide(_ptr(users_t), _ptr(items_t), f, ld, bias, _ptr(uid), args.rows, args.items, None, None, None,
                                                   0, 0, None, None, 0, pool, 0, _ptr(p_items), _ptr(p_scores), _ptr(p_count), _ptr(ws), need,
                                                   _stream()))

        def library():
            _lib.check(lib.wmf_rerank_mmr(_ptr(items_t), args.items, f, ld, bias, _ptr(inv), _ptr(p_items), _ptr(p_scores), _ptr(p_count),
                                          args.rows, pool, args.lam, topn, _ptr(out_items), None, None, None, _stream()))

        def baseline():
            return torch_mmr(items_t, bias, inv, p_items, p_scores, args.lam, topn)

        scan()                                                      # warm up every route at this shape
        library()
        want = baseline()
        scan_runs = [timed(scan)[0] for _ in range(args.reps)]
        lib_runs, torch_runs = [], []
        for _ in range(args.reps):                                  # alternating
            lib_runs.append(timed(library)[0])
            torch_runs.append(timed(baseline)[0])
        lib.wmf_profile_reset()
        lib.wmf_profile_enable(1)
        library()
        torch.cuda.synchronize()
        lib.wmf_profile_enable(0)
        table = [(name, ms) for name, _tag, ms, *_ in _lib.profile_table(lib) if name.startswith("mmr_kernel")]
        lib.wmf_profile_reset()
        same = float((out_items.long() == want).all(dim=1).float().mean())
        is_res = pool <= resident
        nbytes = args.rows * pool * 4 * ld * (1 if is_res else topn - 1)
        row = {"pool": pool, "topn": topn, "kernel": table[0][0] if table else None, "kernel_s": table[0][1] / 1e3 if table else None,
               "variant": "resident" if is_res else "streaming", "bytes_by_the_kernels_count": nbytes,
               "scan": stats(scan_runs), "library": stats(lib_runs), "torch": stats(torch_runs),
               "torch_gather_bytes": args.rows * pool * 4 * (ld - bias), "rows_with_the_same_list": same}
        row["bytes_per_s"] = nbytes / row["library"]["median_s"]
        row["rerank_share_of_scan"] = row["library"]["median_s"] / row["scan"]["median_s"]
        row["torch_over_library"] = row["torch"]["median_s"] / row["library"]["median_s"]
        row["library_faster_beyond_either_spread"] = bool(row["torch"]["median_s"] - row["library"]["median_s"] >
                                                          max(row["torch"]["spread_s"], row["library"]["spread_s"]))
        result["shapes"].append(row)
        print(json.dumps({k: row[k] for k in ("pool", "topn", "kernel", "bytes_per_s", "rerank_share_of_scan", "torch_over_library",
                                              "library_faster_beyond_either_spread", "rows_with_the_same_list")}), flush=True)
        print("  library", row["library"], "\n  torch", row["torch"], "\n  scan", row["scan"], flush=True)
        del ws, p_items, p_scores, p_count, want
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
