"""Timing lab for the neighbours in factor space on a real GPU (not a test): WMF.similar_items -- the catalogue scan with the scaled
scoring rule, wmf_similar_topn -- against two yardsticks in the same process.

Usage: python tools/similar_lab.py [--out FILE] [--reps 5] [queries,items,k,bias,topn ...]

Three paths on the same seeded Gaussian item factors, the queries being the first rows of the catalogue:
  similar    WMF.similar_items(queries, topn), cosine, the row itself left out;
  recommend  WMF.recommend(queries, topn) of a model whose user matrix is those same rows: the same scan with the model's scoring
             rule, the yardstick that already exists;
  dense      what a user has today: normalise with torch, Q @ C^T in blocks of 512 queries, topk.
After a warm-up of each they are timed in alternating repetitions with a host clock that ends in a device synchronise; median and
spread (max - min) per path.  The scan kernels' own times come from the library's wmf_profile_* table, one profiled call of each
fused path per repetition, alternating as well; `similar_dot_scan` is the same kernel with metric='dot' -- no scale arrays, both
factors 1.0f -- which tells the cost of the scale loads from the cost of the rule.  The similar answer is compared with the dense one on the spot: the same rows up to
cosines that agree to 1e-4."""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from recmodel_amd import WMF, _lib  # noqa: E402

DEFAULT_SHAPES = ("2048,1000000,128,1,10", "16,1000000,128,1,10")
DENSE_BLOCK = 512


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "runs_s": ts}


def scan_time(lib, fn, prefix):
    """Seconds the kernels whose name starts with `prefix` took in one call of fn."""
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    timed(fn)
    lib.wmf_profile_enable(0)
    total = sum(ms * 1e-3 for name, _, ms, _, _, _ in _lib.profile_table(lib) if name.startswith(prefix))
    lib.wmf_profile_reset()
    return total


def run_shape(n_queries, n_items, k, bias, topn, reps):
    rng = np.random.default_rng(1000 * k + bias)
    f = k + bias
    items = rng.standard_normal((n_items, f), dtype=np.float32)
    m = WMF(num_items=8, num_users=n_queries, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    m.items, m.users, m.num_items = items, items[:n_queries].copy(), n_items
    m.users.flags.writeable = m.items.flags.writeable = False      # read-only factors: device copies and norms are made once
    queries = np.arange(n_queries)
    feats = torch.from_numpy(items[:, bias:]).cuda()

    def dense():
        C = torch.nn.functional.normalize(feats, dim=1)
        out = []
        for b0 in range(0, n_queries, DENSE_BLOCK):
            s = C[b0: min(b0 + DENSE_BLOCK, n_queries)] @ C.T
            s[torch.arange(s.shape[0]), torch.arange(b0, b0 + s.shape[0])] = -float("inf")       # the row itself
            out.append(torch.topk(s, topn, dim=1))
        return torch.cat([o.indices for o in out]).cpu().numpy(), torch.cat([o.values for o in out]).cpu().numpy()

    similar = lambda: m.similar_items(queries, topn, return_scores=True)  # noqa: E731
    similar_dot = lambda: m.similar_items(queries, topn, metric='dot')  # noqa: E731
    recommend = lambda: m.recommend(queries, topn)  # noqa: E731
    _, (a, sa) = timed(similar)
    timed(recommend)
    timed(similar_dot)
    _, (b, sb) = timed(dense)
    agree = float((a == b).mean())
    score_gap = float(np.abs(np.sort(sa, axis=1) - np.sort(sb, axis=1)).max())
    lib = _lib.load()
    t = {"similar": [], "recommend": [], "dense": [], "similar_scan": [], "recommend_scan": [], "similar_dot_scan": []}
    for _ in range(reps):
        t["similar"].append(timed(similar)[0])
        t["recommend"].append(timed(recommend)[0])
        t["dense"].append(timed(dense)[0])
        t["similar_scan"].append(scan_time(lib, similar, "similar_scan_kernel"))
        t["recommend_scan"].append(scan_time(lib, recommend, "recommend_scan_kernel"))
        t["similar_dot_scan"].append(scan_time(lib, similar_dot, "similar_scan_kernel"))
    rec = {"queries": n_queries, "items": n_items, "k": k, "bias": bias, "topn": topn, **{name: stats(ts) for name, ts in t.items()},
           "norms_s": scan_time(lib, lambda: lib.wmf_row_inv_norms(*norm_args(m)), "row_inv_norms_kernel"),
           "same_rows_as_dense_fraction": agree, "score_gap_to_dense": score_gap}
    gap = rec["similar_scan"]["median_s"] - rec["recommend_scan"]["median_s"]
    rec["scan_gap_s"] = gap
    rec["scan_within_spread"] = bool(gap <= max(rec["similar_scan"]["spread_s"], rec["recommend_scan"]["spread_s"]))
    assert score_gap <= 1e-4, rec
    return rec


def norm_args(m):
    from recmodel_amd.engine import _ptr, _stream
    _, items_t, f, ld = m._device_factors()
    out = torch.empty(items_t.shape[0], dtype=torch.float32, device="cuda")
    m._lab_keep = out
    return _ptr(items_t), items_t.shape[0], f, ld, int(m.bias is True), _ptr(out), _stream()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the full record to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("shapes", nargs="*", default=list(DEFAULT_SHAPES))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[2], "shapes": []}
    for shape in args.shapes:
        n_queries, n_items, k, bias, topn = (int(x) for x in shape.split(","))
        rec = run_shape(n_queries, n_items, k, bias, topn, args.reps)
        out["shapes"].append(rec)
        print(json.dumps({key: rec[key] for key in rec if key != "method"}), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
