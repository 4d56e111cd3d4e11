"""Timing lab for the audit of a half step on a real GPU (not a test): AlsEngine.audit in objective-only mode and with per-row
output, at one configuration of recmodel_amd/synth.py, both sides, after one ALS iteration.

Usage: python tools/audit_lab.py [--config cfg3] [--reps 5] [--out FILE]

After a warm-up of each mode the two are timed in alternating repetitions with a host clock that ends in a device synchronise
(median and spread); the kernels' own times come from the library's wmf_profile_* table (HIP events around every launch).  The
counted bytes of a pass are z (4 f + 8) + n (12 f + 4): every stored entry gathers a float32 row of the fixed side and reads its
index and weight, every row reads its float32 factors and, with per-row output, its float64 dense term."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
from recmodel_amd import WMF, _lib, synth  # noqa: E402
from recmodel_amd.engine import AlsEngine  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_ms(fn):
    lib = _lib.load()
    lib.wmf_profile_reset()
    lib.wmf_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    table = _lib.profile_table(lib)
    lib.wmf_profile_enable(0)
    lib.wmf_profile_reset()
    return {name: round(ms, 4) for name, _, ms, _, _, _ in table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=sorted(synth.CONFIGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_users, n_items, dbar, k, bias = synth.CONFIGS[args.config]
    dev = torch.device("cuda:0")
    indptr, indices, counts = synth.make_counts(n_users, n_items, dbar, 1996, device=dev)
    eng = AlsEngine(n_users, n_items, k, bias, 0.1, device=dev)
    eng.K.confidence_transform(counts, 10.0, 1.0, 0)
    eng.set_interactions(indptr, indices, counts)
    eng.set_factors("items", WMF(num_items=n_items, num_users=1, dim=k, gamma=0.1, weighted=True, bias=bias).items)
    result = {"config": args.config, "f": eng.f, "device": torch.cuda.get_device_name(0), "sides": {}}
    for side in ("users", "items"):
        half = timed(lambda: eng.half_step(side))
        half = min(half, timed(lambda: eng.half_step(side)))
        z, n, f = eng.csr[side].nnz, eng.n_local[side], eng.f
        modes = {"objective_only": lambda: eng.audit(side), "with_rows": lambda: eng.audit(side, rows=True)}
        for fn in modes.values():
            fn()
        runs = {m: [] for m in modes}
        for _ in range(args.reps):
            for m, fn in modes.items():
                runs[m].append(timed(fn))
        audit = eng.audit(side, rows=True)
        eta = audit.pop("eta")
        entry = {"rows": n, "stored_entries": z, "half_step_ms": round(1e3 * half, 3), "counted_bytes": z * (4 * f + 8) + n * (12 * f + 4),
                 "audit": audit, "max_eta": float(eta.max()), "median_eta": float(eta.median())}
        for m, fn in modes.items():
            med = statistics.median(runs[m])
            entry[m] = {"median_ms": round(1e3 * med, 3), "spread_ms": round(1e3 * (max(runs[m]) - min(runs[m])), 3),
                        "counted_GB_per_s": round(entry["counted_bytes"] / med / 1e9, 1), "kernels_ms": kernel_ms(fn)}
        result["sides"][side] = entry
        print(side, json.dumps(entry), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
