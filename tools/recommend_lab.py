"""Timing lab for the full-catalogue recommendation on a real GPU (not a test): WMF.recommend -- one fused scan,
wmf_recommend_topn -- against the path it stands beside, WMF.rank(np.arange(n_items), [users...], topn) -- a score matrix and a
segmented sort, wmf_rank_topn_batch, in batches of 2^26 scores.

Usage: python tools/recommend_lab.py [--out FILE] [--reps 5] [--topn 10] [users,items,k,bias ...]

Both paths run in one process on the same seeded Gaussian factors, without exclusions; after a warm-up of each they are timed
in alternating repetitions with a host clock that ends in a device synchronise; median and spread (max - min) per path.  The two
answers are compared on the spot under the rounded-class rule of the tests: the float64 score of the k-th item of one path is
within B of the k-th of the other.  The fused call is also timed with a seen list of 10 entries per user.  The scan kernel's
own time comes from the library's wmf_profile_* table and is set against max(2 U I ld / f32-MFMA peak, item bytes x passes /
HBM peak) with the peaks of the MI355X data sheet (157.3 TFLOP/s, 8.0 TB/s); passes = blocks of 64 users, each of which
streams the catalogue once."""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, '.')
from recmodel_amd import WMF, _lib  # noqa: E402

MFMA_F32_PEAK, HBM_PEAK = 157.3e12, 8.0e12
DEFAULT_SHAPES = ("2048,100000,64,0", "2048,1000000,128,1", "16,1000000,128,1")
U32 = 2.0 ** -24


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def scores64(m, users, items):
    """float64 scores and the tests' bound B of (users[b], items[b, k])."""
    X, Y = m.users[users].astype(np.float64)[:, None, :], m.items[items].astype(np.float64)
    prod = np.abs(X * Y)
    if m.bias is True:
        s = (X[..., 1:] * Y[..., 1:]).sum(-1) + X[..., 0] + Y[..., 0]
        mass = prod[..., 1:].sum(-1) + np.abs(X[..., 0]) + np.abs(Y[..., 0])
    else:
        s, mass = (X * Y).sum(-1), prod.sum(-1)
    return s, 2.0 * (m.items.shape[1] + 2) * U32 * mass


def stats(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "runs_s": ts}


def run_shape(n_users, n_items, k, bias, topn, reps):
    rng = np.random.default_rng(1000 * k + bias)
    m = WMF(num_items=8, num_users=n_users, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    f = k + bias
    m.users, m.items = rng.standard_normal((n_users, f), dtype=np.float32), rng.standard_normal((n_items, f), dtype=np.float32)
    m.num_items = n_items
    m.users.flags.writeable = m.items.flags.writeable = False      # read-only factors: the device copies are made once
    users = np.arange(n_users)
    everything = np.arange(n_items)
    seen = sp.csr_matrix((np.ones(10 * n_users, dtype=np.float32), rng.integers(0, n_items, 10 * n_users), 10 * np.arange(n_users + 1)),
                         shape=(n_users, n_items))
    fused = lambda: m.recommend(users, topn)  # noqa: E731
    fused_seen = lambda: m.recommend(users, topn, exclude=seen)  # noqa: E731
    parent = lambda: np.stack(m.rank(everything, list(users), topn=topn))  # noqa: E731
    _, a = timed(fused)
    timed(fused_seen)
    _, b = timed(parent)
    # the two answers under the rounded-class rule
    sa, ba = scores64(m, users, a)
    sb, bb = scores64(m, users, b)
    ratio = float((np.abs(sa - sb) / np.maximum(ba, bb)).max())
    t = {"fused": [], "parent": [], "fused_seen10": []}
    for _ in range(reps):
        t["fused"].append(timed(fused)[0])
        t["parent"].append(timed(parent)[0])
        t["fused_seen10"].append(timed(fused_seen)[0])
    # the kernels' own time
    lib = _lib.load()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    timed(fused)
    lib.wmf_profile_enable(0)
    kernels = {name: ms / max(n, 1) * 1e-3 for name, _, ms, n, _, _ in _lib.profile_table(lib)}
    calls = {name: n for name, _, _, n, _, _ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    scan = sum(kernels[nm] * calls[nm] for nm in kernels if nm.startswith("recommend_scan_kernel"))
    ld = int(lib.wmf_ld_for(f))
    mfma_s = 2.0 * n_users * n_items * ld / MFMA_F32_PEAK
    hbm_s = n_items * ld * 4.0 * ((n_users + 63) // 64) / HBM_PEAK
    rec = {"users": n_users, "items": n_items, "k": k, "bias": bias, "topn": topn,
           "fused": stats(t["fused"]), "parent": stats(t["parent"]), "fused_seen10": stats(t["fused_seen10"]),
           "same_items_fraction": float((a == b).mean()), "order_gap_over_bound": ratio,
           "kernel_s": {nm: kernels[nm] * calls[nm] for nm in kernels},
           "scan_bound_s": max(mfma_s, hbm_s), "scan_bound_term": "f32 MFMA" if mfma_s >= hbm_s else "HBM",
           "scan_share_of_bound": (max(mfma_s, hbm_s) / scan) if scan else None}
    gap = rec["parent"]["median_s"] - rec["fused"]["median_s"]
    rec["fused_faster_beyond_spread"] = bool(gap > max(rec["parent"]["spread_s"], rec["fused"]["spread_s"]))
    assert ratio <= 1.0, rec
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the full record to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("shapes", nargs="*", default=list(DEFAULT_SHAPES))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[2], "shapes": []}
    for shape in args.shapes:
        n_users, n_items, k, bias = (int(x) for x in shape.split(","))
        rec = run_shape(n_users, n_items, k, bias, args.topn, args.reps)
        out["shapes"].append(rec)
        print(json.dumps({key: rec[key] for key in ("users", "items", "k", "bias", "fused", "parent", "fused_seen10", "kernel_s",
                                                     "scan_share_of_bound", "scan_bound_term", "same_items_fraction")}), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
