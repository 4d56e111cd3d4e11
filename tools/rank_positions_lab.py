"""Timing lab for the exact full-catalogue ranks on a real GPU (not a test): WMF.rank_positions -- one counting scan,
wmf_rank_positions -- against the only route to the same ranks without it, WMF.rank(unseen, u, topn=None) user by user and a
look-up of the held-out items in the returned order, and beside its peer, WMF.recommend(topn=10) at the same shape.

Usage: python tools/rank_positions_lab.py [--out FILE] [--reps 5] [--sample 16] [users,items,k,bias ...]

Everything runs in one process on the same seeded Gaussian factors, with 10 seen items and 5 held-out items per user; after a
warm-up of each path they are timed in alternating repetitions with a host clock that ends in a device synchronise; median and
spread (max - min) per path.  The per-user route is run on a sample of the users small enough to finish, and the new path on the
same sample beside it: that pair is the gated comparison (new median below the route's by more than both spreads).  The new path
on all users stands beside recommend(topn=10) on all users; their ratio is reported, not gated.  Held-out items are STRONG (five of
the user's own 128 best unseen items, what a trained model's test items look like: nearly every score fails the early-out) and,
as the worst case for the early-out on record, UNIFORM over the catalogue (most scores pass it and are placed among the target
keys).  The kernels' own times come from the library's wmf_profile_* table."""
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

DEFAULT_SHAPES = ("2048,100000,64,0", "2048,1000000,128,1", "16,1000000,128,1")
N_SEEN, N_TARGETS = 10, 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "runs_s": ts}


def by_rank(m, held_out, seen, users):
    """The ranks of the held-out items through rank(unseen, u, topn=None), user by user."""
    n_items = m.items.shape[0]
    everything = np.arange(n_items, dtype=np.int32)
    out = []
    for u in users:
        unseen = np.delete(everything, seen.indices[seen.indptr[u]:seen.indptr[u + 1]])
        place = np.full(n_items, -1, dtype=np.int64)
        order = m.rank(unseen, int(u), topn=None)
        place[order] = np.arange(len(order))
        out.append(place[held_out.indices[held_out.indptr[u]:held_out.indptr[u + 1]]])
    return np.concatenate(out)


def kernel_times(fn):
    lib = _lib.load()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    timed(fn)
    lib.wmf_profile_enable(0)
    table = {name: ms * 1e-3 for name, _, ms, _, _, _ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return table


def run_shape(n_users, n_items, k, bias, reps, sample):
    rng = np.random.default_rng(1000 * k + bias)
    m = WMF(num_items=8, num_users=n_users, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    f = k + bias
    m.users, m.items = rng.standard_normal((n_users, f), dtype=np.float32), rng.standard_normal((n_items, f), dtype=np.float32)
    m.num_items = n_items
    m.users.flags.writeable = m.items.flags.writeable = False      # read-only factors: the device copies are made once
    users = np.arange(n_users)
    some = users[:min(sample, n_users)]

    def rows(cols):
        mat = sp.csr_matrix((np.ones(cols.size, dtype=np.float32), cols.reshape(-1), cols.shape[1] * np.arange(n_users + 1)), shape=(n_users, n_items))
        mat.sum_duplicates()
        return mat
    seen = rows(rng.integers(0, n_items, (n_users, N_SEEN)))
    best = m.recommend(users, 128, exclude=seen)
    held = {"strong": rows(np.stack([rng.permutation(row)[:N_TARGETS] for row in best])),
            "uniform": rows(rng.integers(0, n_items, (n_users, N_TARGETS)))}
    rec = {"users": n_users, "items": n_items, "k": k, "bias": bias, "seen_per_user": N_SEEN, "targets_per_user": N_TARGETS,
           "sample_users": len(some)}
    peer = lambda: m.recommend(users, 10, exclude=seen)  # noqa: E731
    timed(peer)
    for kind, held_out in held.items():
        new_all = lambda: m.rank_positions(held_out, exclude=seen)  # noqa: E731
        new_some = lambda: m.rank_positions(held_out, exclude=seen, users=some)  # noqa: E731
        route = lambda: by_rank(m, held_out, seen, some)  # noqa: E731
        _, (_, _, ranks_all) = timed(new_all)
        _, (_, _, a) = timed(new_some)
        _, b = timed(route)
        t = {"new_all_users": [], "recommend_top10_all_users": [], "new_sample": [], "rank_route_sample": []}
        for _ in range(reps):
            t["new_all_users"].append(timed(new_all)[0])
            t["recommend_top10_all_users"].append(timed(peer)[0])
            t["new_sample"].append(timed(new_some)[0])
            t["rank_route_sample"].append(timed(route)[0])
        r = {key: stats(v) for key, v in t.items()}
        # rank() sums a score in another order than the MFMA tiles: a one-ulp difference may move a place, so the two
        # routes are set side by side, not asserted equal
        r["sample_ranks_equal_fraction"] = float((a == b).mean())
        r["sample_ranks_max_abs_difference"] = int(np.abs(a - b).max())
        r["median_rank"] = float(np.median(ranks_all[ranks_all >= 0]))
        gap = r["rank_route_sample"]["median_s"] - r["new_sample"]["median_s"]
        r["new_faster_beyond_both_spreads"] = bool(gap > max(r["rank_route_sample"]["spread_s"], r["new_sample"]["spread_s"]))
        r["rank_route_extrapolated_to_all_users_s"] = r["rank_route_sample"]["median_s"] * n_users / len(some)
        r["new_over_recommend_top10"] = r["new_all_users"]["median_s"] / r["recommend_top10_all_users"]["median_s"]
        r["kernel_s"] = kernel_times(new_all)
        rec[kind] = r
    rec["recommend_kernel_s"] = kernel_times(peer)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the full record to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16, help="users of the per-user rank() route")
    ap.add_argument("shapes", nargs="*", default=list(DEFAULT_SHAPES))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[2], "shapes": []}
    for shape in args.shapes:
        n_users, n_items, k, bias = (int(x) for x in shape.split(","))
        rec = run_shape(n_users, n_items, k, bias, args.reps, args.sample)
        out["shapes"].append(rec)
        for kind in ("strong", "uniform"):
            r = rec[kind]
            print(json.dumps({"users": n_users, "items": n_items, "k": k, "bias": bias, "targets": kind,
                              **{key: {"median_s": r[key]["median_s"], "spread_s": r[key]["spread_s"]}
                                 for key in ("new_all_users", "recommend_top10_all_users", "new_sample", "rank_route_sample")},
                              "new_faster_beyond_both_spreads": r["new_faster_beyond_both_spreads"],
                              "new_over_recommend_top10": r["new_over_recommend_top10"], "median_rank": r["median_rank"],
                              "sample_ranks_equal_fraction": r["sample_ranks_equal_fraction"], "kernel_s": r["kernel_s"]}), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
