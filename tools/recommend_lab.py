"""Timing lab for the full-catalogue recommendation on a real GPU (not a test): WMF.recommend -- one fused scan,
wmf_recommend_topn -- against the path it stands beside, WMF.rank(np.arange(n_items), [users...], topn) -- a score matrix and a
segmented sort, wmf_rank_topn_batch, in batches of 2^26 scores.

Usage: python tools/recommend_lab.py [--out FILE] [--reps 5] [--topn 10] [users,items,k,bias ...]
       python tools/recommend_lab.py --filters [--out FILE] [--reps 5] [--topn 10] [users,items,k,bias]
       python tools/recommend_lab.py --wide [--out FILE] [--reps 5] [items,k,bias]

Both paths run in one process on the same seeded Gaussian factors, without exclusions; after a warm-up of each they are timed
in alternating repetitions with a host clock that ends in a device synchronise; median and spread (max - min) per path.  The two
answers are compared on the spot under the rounded-class rule of the tests: the float64 score of the k-th item of one path is
within B of the k-th of the other.  The fused call is also timed with a seen list of 10 entries per user.  The scan kernel's
own time comes from the library's wmf_profile_* table and is set against max(2 U I ld / f32-MFMA peak, item bytes x passes /
HBM peak) with the peaks of the MI355X data sheet (157.3 TFLOP/s, 8.0 TB/s); passes = blocks of 64 users, each of which
streams the catalogue once.

--filters: the catalogue filters of WMF.recommend (wmf_recommend_topn_filtered) at one shape, with a seen list of 10 entries per
user, at pass rates of 50 %, 1 % and 0.01 % of the catalogue: the mask form and the list form next to the unfiltered call (the
parent's scan kernel, unchanged) in alternating repetitions of one process, and the two routes a caller had before -- the
complement of the filter appended to ``exclude`` through the unfiltered call, for the first COMPLEMENT_USERS users (for all of them
the seen list would be about 8 GB), and rank(allowed, users, topn), which knows no seen items.  The answers are compared on the
spot: filtered against complement-in-exclude bit for bit, rank under the rounded-class rule against the list form without a seen
list.  Then the list form at a ladder of list lengths against the mask form of the same list: where the two cross.

--wide: WMF.candidates and the device path of WMF.recommend beyond 128 (wmf_recommend_topn_wide) at 1 000 000 items, k = 128 +
biases, 10 seen items per row, 2048 and 16 users, every pair of routes in alternating repetitions of one process: (1) 16 users at
topn 200, this commit's recommend against the parent's, the host loop over rank() and predict(), which is still the code beyond
CANDIDATES_MAX and is reached by lowering that constant for the call; (2) topn 128 through wmf_recommend_topn and through the wide
kernels, scan and selection kernel apart from the library's wmf_profile_* table; (3) the ladder topn 129 .. 4096 with the automatic
slice count, the workspace and the rows of a call; (4) the mask form at a 1 % pass rate and the list form of 10 000 ids at topn 1000.

--shelves: WMF.recommend_shelves (wmf_recommend_topn_grouped, one scan for all shelves) at 1 000 000 items, k = 128 + biases, 10 seen
items per row, topn 10, shelves assigned j % G and, once, Zipf-sized: against the route it replaces -- WMF.recommend with every user
repeated once per shelf under G masks (wmf_recommend_topn_filtered; at 64 shelves on 256 of the 2048 users and scaled, which the
record says) -- and against one unfiltered wide scan at topn 10 (WMF.candidates), the floor.  The three routes of a shape in
alternating repetitions of one process after a warm-up of each, a host clock ending in a synchronise, median and spread; the arrays
of the first two compared for identity; scan and selection kernel apart from the library's wmf_profile_* table.  The gate: at 2048
users and 16 shelves the new call's median is below the repeated rows' by more than the larger spread, and the arrays are identical."""
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


COMPLEMENT_USERS = 128
PASS_RATES = (0.5, 0.01, 0.0001)
LADDER = (1000, 10000, 100000, 250000, 500000, 750000, 1000000)


def scan_kernel_s(lib, fn):
    """{kernel: seconds} of one call of fn, from the library's own event table."""
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    timed(fn)
    lib.wmf_profile_enable(0)
    out = {name: ms * 1e-3 for name, _, ms, _, _, _ in _lib.profile_table(lib)}
    lib.wmf_profile_reset()
    return out


def same_bits(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)))


def run_filters(n_users, n_items, k, bias, topn, reps):
    rng = np.random.default_rng(1000 * k + bias)
    m = WMF(num_items=8, num_users=n_users, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    f = k + bias
    m.users, m.items = rng.standard_normal((n_users, f), dtype=np.float32), rng.standard_normal((n_items, f), dtype=np.float32)
    m.num_items = n_items
    m.users.flags.writeable = m.items.flags.writeable = False
    users = np.arange(n_users)
    seen = sp.csr_matrix((np.ones(10 * n_users, dtype=np.float32), rng.integers(0, n_items, 10 * n_users), 10 * np.arange(n_users + 1)),
                         shape=(n_users, n_items))
    seen.sum_duplicates()
    lib = _lib.load()
    few = users[:min(COMPLEMENT_USERS, n_users)]
    unfiltered = lambda: m.recommend(users, topn, exclude=seen, return_scores=True)  # noqa: E731
    timed(unfiltered)
    rec = {"users": n_users, "items": n_items, "k": k, "bias": bias, "topn": topn, "seen_per_user": 10,
           "complement_users": len(few), "rates": [], "ladder": []}
    for rate in PASS_RATES:
        mask = rng.random(n_items) < rate
        ids = np.flatnonzero(mask)
        comp = np.flatnonzero(~mask)
        rows = [np.union1d(comp, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]) for u in few]
        big = sp.csr_matrix((np.ones(sum(len(r) for r in rows), dtype=np.float32), np.concatenate(rows),
                             np.concatenate([[0], np.cumsum([len(r) for r in rows])])), shape=(len(few), n_items))
        big.resize((n_users, n_items))                              # (rows past the first complement_users stay empty and are not asked for)
        routes = {"unfiltered": unfiltered,
                  "mask": lambda: m.recommend(users, topn, exclude=seen, return_scores=True, allow=mask),
                  "list": lambda: m.recommend(users, topn, exclude=seen, return_scores=True, allow=ids),
                  "mask_few_users": lambda: m.recommend(few, topn, exclude=seen, return_scores=True, allow=mask),
                  "complement_in_exclude_few_users": lambda: m.recommend(few, topn, exclude=big, return_scores=True),
                  "rank_allowed_no_seen": lambda: np.stack(m.rank(ids, list(users), topn=min(topn, len(ids))))}
        first = {}
        for name, fn in routes.items():                            # (the warm-up of each route; its time is not used)
            dt, first[name] = timed(fn)
            print(f"# pass rate {rate}: {name} warmed up in {dt:.3f} s", file=sys.stderr, flush=True)
        agree = {"mask_equals_list_bits": same_bits(first["mask"], first["list"]),
                 "mask_equals_complement_in_exclude_bits": same_bits(first["mask_few_users"], first["complement_in_exclude_few_users"]),
                 "list_equals_complement_in_exclude_bits": same_bits([a[:len(few)] for a in first["list"]], first["complement_in_exclude_few_users"])}
        no_seen = m.recommend(users, min(topn, len(ids)), allow=ids)
        sa, ba = scores64(m, users, no_seen)
        sb, bb = scores64(m, users, first["rank_allowed_no_seen"])
        agree["rank_order_gap_over_bound"] = float((np.abs(sa - sb) / np.maximum(ba, bb)).max())
        agree["rank_same_items_fraction"] = float((no_seen == first["rank_allowed_no_seen"]).mean())
        assert all(v for key, v in agree.items() if key.endswith("_bits")) and agree["rank_order_gap_over_bound"] <= 1.0, agree
        t = {name: [] for name in routes}
        for _ in range(reps):
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
        entry = {"pass_rate": rate, "allowed": int(len(ids)), "agreement": agree, **{name: stats(ts) for name, ts in t.items()},
                 "kernel_s": {name: scan_kernel_s(lib, routes[name]) for name in ("unfiltered", "mask", "list")}}
        scan = {name: sum(v for nm, v in entry["kernel_s"][name].items() if nm.startswith("recommend_scan")) for name in entry["kernel_s"]}
        entry["scan_kernel_s"] = scan
        entry["mask_over_unfiltered"] = {"call": entry["mask"]["median_s"] / entry["unfiltered"]["median_s"], "scan_kernel": scan["mask"] / scan["unfiltered"]}
        entry["list_over_unfiltered"] = {"call": entry["list"]["median_s"] / entry["unfiltered"]["median_s"], "scan_kernel": scan["list"] / scan["unfiltered"]}
        rec["rates"].append(entry)
        print(json.dumps({key: entry[key] for key in ("pass_rate", "allowed", "agreement", "scan_kernel_s", "mask_over_unfiltered", "list_over_unfiltered")}
                         | {name: entry[name]["median_s"] for name in routes}), flush=True)
        del big, rows, comp
    # where the two forms cross: the same list through both, at a ladder of lengths
    order = rng.permutation(n_items)
    for n_cand in [n for n in LADDER if n <= n_items]:
        ids = np.sort(order[:n_cand])
        mask = np.zeros(n_items, dtype=bool)
        mask[ids] = True
        forms = {"mask": lambda: m.recommend(users, topn, exclude=seen, return_scores=True, allow=mask),
                 "list": lambda: m.recommend(users, topn, exclude=seen, return_scores=True, allow=ids)}
        assert same_bits(timed(forms["mask"])[1], timed(forms["list"])[1])
        t = {name: [] for name in forms}
        for _ in range(reps):
            for name, fn in forms.items():
                t[name].append(timed(fn)[0])
        kern = {name: sum(v for nm, v in scan_kernel_s(lib, fn).items() if nm.startswith("recommend_scan")) for name, fn in forms.items()}
        rec["ladder"].append({"n_cand": n_cand, "mask": stats(t["mask"]), "list": stats(t["list"]), "scan_kernel_s": kern})
        print(json.dumps({"n_cand": n_cand, "mask_s": rec["ladder"][-1]["mask"]["median_s"], "list_s": rec["ladder"][-1]["list"]["median_s"],
                          "scan_kernel_s": kern}), flush=True)
    for key, pick in (("call", lambda e, nm: e[nm]["median_s"]), ("scan_kernel", lambda e, nm: e["scan_kernel_s"][nm])):
        cross = None
        for lo, hi in zip(rec["ladder"], rec["ladder"][1:]):
            d0, d1 = pick(lo, "list") - pick(lo, "mask"), pick(hi, "list") - pick(hi, "mask")
            if d0 < 0 <= d1:
                cross = lo["n_cand"] + (hi["n_cand"] - lo["n_cand"]) * (-d0) / (d1 - d0)
        rec[f"crossover_n_cand_by_{key}"] = cross
        rec[f"list_faster_at_every_length_by_{key}"] = bool(all(pick(e, "list") < pick(e, "mask") for e in rec["ladder"]))
    return rec


WIDE_LADDER = (129, 256, 512, 1000, 2048, 4096)
WIDE_USERS = (2048, 16)


def wide_slices(n_users, n_scan, topn):
    """The automatic slice count of wmf_recommend_topn_wide, from the constants and the rule of include/wmf_hip.h."""
    import re
    header = open("include/wmf_hip.h").read()
    c = {n: int(re.search(rf"#define\s+WMF_RECOMMEND_WIDE_{n}\s+(\d+)", header).group(1)) for n in ("AUTO_SLICES", "AUTO_LISTS", "SLICE_TOPNS")}
    s0 = min(c["AUTO_SLICES"] * n_users, max(c["AUTO_LISTS"], n_users)) // n_users
    slice_items = max(1024, c["SLICE_TOPNS"] * topn)
    return max(1, min(s0, -(-((n_scan + 15) // 16) // -(-slice_items // 16))))


def kernel_split(lib, fn):
    """(scan seconds, selection or merge seconds, names) of one call of fn."""
    k = scan_kernel_s(lib, fn)
    return (sum(v for nm, v in k.items() if nm.startswith("recommend_scan")),
            sum(v for nm, v in k.items() if nm.startswith(("recommend_select", "recommend_merge"))), sorted(k))


def alternate(routes, reps):
    """{name: stats} of the routes timed in alternating repetitions, after one warm-up each."""
    for fn in routes.values():
        timed(fn)
    t = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t[name].append(timed(fn)[0])
    return {name: stats(ts) for name, ts in t.items()}


def run_wide(n_items, k, bias, reps):
    from recmodel_amd import wmf_model
    rng = np.random.default_rng(1000 * k + bias)
    f = k + bias
    n_all = max(WIDE_USERS)
    m = WMF(num_items=8, num_users=n_all, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    m.users, m.items = rng.standard_normal((n_all, f), dtype=np.float32), rng.standard_normal((n_items, f), dtype=np.float32)
    m.num_items = n_items
    m.users.flags.writeable = m.items.flags.writeable = False
    seen = sp.csr_matrix((np.ones(10 * n_all, dtype=np.float32), rng.integers(0, n_items, 10 * n_all), 10 * np.arange(n_all + 1)),
                         shape=(n_all, n_items))
    seen.sum_duplicates()
    lib = _lib.load()
    rec = {"items": n_items, "k": k, "bias": bias, "seen_per_user": 10}

    # 1. the gate: 16 users, topn 200, the parent's host loop against the device path
    few = np.arange(16)

    def parent_200():
        limit = wmf_model.CANDIDATES_MAX
        wmf_model.CANDIDATES_MAX = wmf_model.RECOMMEND_MAX_TOPN        # the parent's routing: beyond 128, user by user
        try:
            return m.recommend(few, 200, exclude=seen, return_scores=True)
        finally:
            wmf_model.CANDIDATES_MAX = limit
    new_200 = lambda: m.recommend(few, 200, exclude=seen, return_scores=True)  # noqa: E731
    a, b = parent_200(), new_200()
    sa, ba = scores64(m, few, a[0])
    sb, bb = scores64(m, few, b[0])
    gate = alternate({"parent_host_loop": parent_200, "wide_device_path": new_200}, reps)
    gate["same_items_fraction"] = float((a[0] == b[0]).mean())
    gate["order_gap_over_bound"] = float((np.abs(sa - sb) / np.maximum(ba, bb)).max())
    gate["parent_over_wide"] = gate["parent_host_loop"]["median_s"] / gate["wide_device_path"]["median_s"]
    gate["wide_faster_beyond_spread"] = bool(gate["parent_host_loop"]["median_s"] - gate["wide_device_path"]["median_s"]
                                             > max(gate["parent_host_loop"]["spread_s"], gate["wide_device_path"]["spread_s"]))
    assert gate["order_gap_over_bound"] <= 1.0, gate
    rec["topn200_16_users"] = gate
    print(json.dumps({"topn200_16_users": {key: (v["median_s"] if isinstance(v, dict) else v) for key, v in gate.items()}}), flush=True)

    # 2. the price of the workspace buffers at topn 128, and 3. the ladder
    rec["topn128"], rec["ladder"] = [], []
    for n_users in WIDE_USERS:
        users = np.arange(n_users)
        routes = {"fused": lambda: m.recommend(users, 128, exclude=seen, return_scores=True),
                  "wide": lambda: m.candidates(users, 128, exclude=seen, return_scores=True)}
        assert same_bits(routes["fused"](), routes["wide"]())
        entry = {"users": n_users, **alternate(routes, reps)}
        for name, fn in routes.items():
            scan, tail, names = kernel_split(lib, fn)
            entry[name + "_kernels"] = {"scan_s": scan, "select_or_merge_s": tail, "names": names}
        entry["wide_scan_over_fused_scan"] = entry["wide_kernels"]["scan_s"] / entry["fused_kernels"]["scan_s"]
        rec["topn128"].append(entry)
        print(json.dumps({key: (v["median_s"] if isinstance(v, dict) and "median_s" in v else v) for key, v in entry.items()}), flush=True)
        for topn in WIDE_LADDER:
            fn = lambda: m.candidates(users, topn, exclude=seen, return_scores=True)  # noqa: E731
            rows = n_users
            while rows > 1 and lib.wmf_recommend_wide_workspace_bytes(rows, topn, 0) > wmf_model.CANDIDATES_WS_BYTES:
                rows //= 2
            step = {"users": n_users, "topn": topn, "rows_per_call": rows, "auto_slices": wide_slices(rows, n_items, topn),
                    "workspace_bytes": int(lib.wmf_recommend_wide_workspace_bytes(rows, topn, 0)), **alternate({"call": fn}, reps)}
            step["scan_s"], step["select_s"], _ = kernel_split(lib, fn)
            rec["ladder"].append(step)
            print(json.dumps({key: (v["median_s"] if isinstance(v, dict) else v) for key, v in step.items()}), flush=True)

    # 4. the filtered forms at topn 1000
    users = np.arange(n_all)
    mask = rng.random(n_items) < 0.01
    ids = np.sort(rng.choice(n_items, 10000, replace=False))
    routes = {"unfiltered": lambda: m.candidates(users, 1000, exclude=seen, return_scores=True),
              "mask_1_percent": lambda: m.candidates(users, 1000, exclude=seen, return_scores=True, allow=mask),
              "list_10000_ids": lambda: m.candidates(users, 1000, exclude=seen, return_scores=True, allow=ids)}
    filt = {"users": n_all, "topn": 1000, "mask_allowed": int(mask.sum()), **alternate(routes, reps)}
    for name, fn in routes.items():
        scan, tail, names = kernel_split(lib, fn)
        filt[name + "_kernels"] = {"scan_s": scan, "select_s": tail, "names": names}
    list_mask = np.zeros(n_items, dtype=bool)
    list_mask[ids] = True
    filt["list_equals_its_mask_bits"] = same_bits(routes["list_10000_ids"](), m.candidates(users, 1000, exclude=seen, return_scores=True, allow=list_mask))
    assert filt["list_equals_its_mask_bits"]
    rec["filters_topn1000"] = filt
    print(json.dumps({key: (v["median_s"] if isinstance(v, dict) and "median_s" in v else v) for key, v in filt.items()}), flush=True)
    return rec


SHELF_SHAPES = ((2048, 1, "mod"), (2048, 2, "mod"), (2048, 4, "mod"), (2048, 16, "mod"), (2048, 16, "zipf"), (2048, 64, "mod"), (16, 16, "mod"))
SHELF_SCALED_ROWS = 256             # rows of the repeated-rows route at 64 shelves (2048 x 64 rows would be 64 scans a repetition)


def run_shelves(n_items, k, bias, topn, reps):
    rng = np.random.default_rng(1000 * k + bias)
    f = k + bias
    n_all = max(s[0] for s in SHELF_SHAPES)
    m = WMF(num_items=8, num_users=n_all, dim=k, gamma=0.1, weighted=True, bias=bool(bias))
    m.users, m.items = rng.standard_normal((n_all, f), dtype=np.float32), rng.standard_normal((n_items, f), dtype=np.float32)
    m.num_items = n_items
    m.users.flags.writeable = m.items.flags.writeable = False
    seen = sp.csr_matrix((np.ones(10 * n_all, dtype=np.float32), rng.integers(0, n_items, 10 * n_all), 10 * np.arange(n_all + 1)),
                         shape=(n_all, n_items))
    seen.sum_duplicates()
    lib = _lib.load()
    rec = {"items": n_items, "k": k, "bias": bias, "topn": topn, "seen_per_user": 10, "shapes": []}
    for n_users, G, how in SHELF_SHAPES:
        if how == "mod":
            groups = np.arange(n_items) % G
        else:                                                       # Zipf-sized shelves: shelf g holds a share proportional to 1 / (g + 1)
            share = 1.0 / np.arange(1, G + 1)
            groups = rng.permutation(np.minimum(np.searchsorted(np.cumsum(share / share.sum()), (np.arange(n_items) + 0.5) / n_items), G - 1))
        groups.flags.writeable = False
        masks = np.stack([groups == g for g in range(G)])
        users = np.arange(n_users)
        rows_b = n_users if G < 64 else min(n_users, SHELF_SCALED_ROWS)
        rep, idx = np.repeat(users[:rows_b], G), np.tile(np.arange(G), rows_b)
        routes = {"shelves": lambda: m.recommend_shelves(users, groups, topn, exclude=seen, return_scores=True),
                  "repeated_rows": lambda: m.recommend(rep, topn, exclude=seen, return_scores=True, allow=masks, allow_idx=idx),
                  "one_wide_scan": lambda: m.candidates(users, topn, exclude=seen, return_scores=True)}
        a, b = routes["shelves"](), routes["repeated_rows"]()
        entry = {"users": n_users, "groups": G, "assignment": how, "group_sizes_min_max": [int(np.bincount(groups).min()), int(np.bincount(groups).max())],
                 "repeated_rows_users": rows_b, "repeated_rows_scaled": rows_b != n_users,
                 "identical_arrays": same_bits([x[:rows_b].reshape(rows_b * G, topn) for x in a], b), **alternate(routes, reps)}
        assert entry["identical_arrays"], (n_users, G, how)
        for name, fn in routes.items():
            scan, tail, names = kernel_split(lib, fn)
            entry[name + "_kernels"] = {"scan_s": scan, "select_or_merge_s": tail, "names": names}
        med = {name: entry[name]["median_s"] for name in routes}
        entry["shelves_over_one_wide_scan"] = med["shelves"] / med["one_wide_scan"]
        entry["shelves_scan_over_wide_scan"] = entry["shelves_kernels"]["scan_s"] / entry["one_wide_scan_kernels"]["scan_s"]
        entry["repeated_rows_over_shelves"] = med["repeated_rows"] * (n_users / rows_b) / med["shelves"]
        entry["shelves_faster_beyond_spread"] = bool(not entry["repeated_rows_scaled"] and med["repeated_rows"] - med["shelves"]
                                                     > max(entry["shelves"]["spread_s"], entry["repeated_rows"]["spread_s"]))
        rec["shapes"].append(entry)
        print(json.dumps({key: (v["median_s"] if isinstance(v, dict) and "median_s" in v else v) for key, v in entry.items()
                          if not key.endswith("_kernels")}), flush=True)
    gate = next(e for e in rec["shapes"] if (e["users"], e["groups"], e["assignment"]) == (2048, 16, "mod"))
    rec["gate"] = {"shape": "2048 users, 16 shelves", "passed": bool(gate["shelves_faster_beyond_spread"] and gate["identical_arrays"]),
                   "shelves_median_s": gate["shelves"]["median_s"], "repeated_rows_median_s": gate["repeated_rows"]["median_s"]}
    rec["repeated_rows_wins_at_groups"] = [e["groups"] for e in rec["shapes"]
                                           if e["users"] == 2048 and not e["repeated_rows_scaled"] and e["repeated_rows"]["median_s"] < e["shelves"]["median_s"]]
    print(json.dumps({"gate": rec["gate"], "repeated_rows_wins_at_groups": rec["repeated_rows_wins_at_groups"]}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the full record to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--filters", action="store_true", help="the catalogue filters at one shape (default 2048,1000000,128,1)")
    ap.add_argument("--wide", action="store_true", help="candidates() and recommend() beyond 128 (default 1000000,128,1)")
    ap.add_argument("--shelves", action="store_true", help="recommend_shelves() against repeated rows under masks (default 1000000,128,1)")
    ap.add_argument("shapes", nargs="*", default=None)
    args = ap.parse_args()
    if args.shelves:
        n_items, k, bias = (int(x) for x in (args.shapes or ["1000000,128,1"])[0].split(","))
        out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[5], "shelves": run_shelves(n_items, k, bias, args.topn, args.reps)}
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
        return
    if args.wide:
        n_items, k, bias = (int(x) for x in (args.shapes or ["1000000,128,1"])[0].split(","))
        out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[4], "wide": run_wide(n_items, k, bias, args.reps)}
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
        return
    if args.filters:
        n_users, n_items, k, bias = (int(x) for x in (args.shapes or [DEFAULT_SHAPES[1]])[0].split(","))
        out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[3],
               "filters": run_filters(n_users, n_items, k, bias, args.topn, args.reps)}
        print(json.dumps({key: out["filters"][key] for key in out["filters"] if key.startswith(("crossover", "list_faster"))}), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
        return
    args.shapes = args.shapes or list(DEFAULT_SHAPES)
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
