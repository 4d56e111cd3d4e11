#!/usr/bin/env python3
"""The outputs of the four calls on a row's own system (csrc/wmf_rowsystem.h) as bits: the check that a change to the shared text
left wmf_explain_rows, wmf_foldin_rows, wmf_posterior_draw_rows and wmf_posterior_score_rows alone.

    WMF_HIP_LIB=<one build> python tools/rowsystem_bits.py dump a.npz
    WMF_HIP_LIB=<another>   python tools/rowsystem_bits.py dump b.npz        (a fresh process: the library is loaded once)
    python tools/rowsystem_bits.py compare a.npz b.npz                       (no GPU; exit status 1 unless every array is identical)

dump runs every case of tests/explain_ref.py (explain), tests/foldin_ref.py (fold-in; draws at sigma = 0 on posterior_ref's
identity cases) and posterior_ref's gated cases (1, 16 and 17 draws at sigma = 0.5; 1, 16 and 17 targets), and three rows of unit
vectors whose middle one is not positive definite, and writes every output array whole, padding included.  compare is byte for
byte, NaN payloads included.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DRAW_COUNTS = TARGET_COUNTS = (1, 16, 17)
SIGMA, SEED = 0.5, 7


def indefinite_case():
    """Unit vectors as items, the identity as W_white: the entry (item 3, -3) makes the middle row's pivot 1 - 3."""
    import explain_ref
    f, ld = 8, 12
    values = np.random.default_rng(3).uniform(1, 5, 9).astype(np.float32)
    values[3] = -3.0
    eye = explain_ref.padded(np.eye(f, dtype=np.float32), ld)
    return dict(f=f, ld=ld, bias=0, m=f, Y=eye, W32=eye, indptr=np.array([0, 3, 5, 9], dtype=np.int64),
                indices=np.array([0, 1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int32), values=values,
                targets=np.array([[0, 3, -1, 7]] * 3, dtype=np.int32))


def dump(path):
    import torch

    import explain_ref
    import foldin_ref
    import posterior_ref
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    _lib.require_gpu()
    lib = _lib.load()
    out = {}

    def dev(a, dtype):
        return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()

    def run(c, key, explain=None, foldin=False, draws=(), sigma=SIGMA, targets=()):
        n, f, ld = len(c["indptr"]) - 1, c["f"], c["ld"]
        Y, W, ip = dev(c["Y"], np.float32), dev(c["W32"], np.float32), dev(c["indptr"], np.int64)
        idx, vals = dev(np.append(c["indices"], 0), np.int32), dev(np.append(c["values"], 0), np.float32)
        head = (_ptr(Y), c["m"], f, ld, c["bias"], _ptr(W), _ptr(ip), _ptr(idx), _ptr(vals), n)
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(256, dtype=torch.uint8, device="cuda")
        tail = (_ptr(fail), _ptr(ws), 256, _stream())

        def filled(*shape):
            return torch.full(shape, -12345.0, dtype=torch.float32, device="cuda")
        if explain is not None:
            T = explain.shape[1]
            contrib, total = filled(len(c["indices"]) + 1, T), filled(n, T)
            _lib.check(lib.wmf_explain_rows(*head, _ptr(dev(explain, np.int32)), T, _ptr(contrib), _ptr(total), *tail))
            out[f"{key}/contrib"], out[f"{key}/total"] = contrib.cpu().numpy(), total.cpu().numpy()
        if foldin:
            X = filled(n, ld)
            _lib.check(lib.wmf_foldin_rows(*head, _ptr(X), *tail))
            out[f"{key}/foldin"] = X.cpu().numpy()
        for D in draws:
            X = filled(n * D, ld)
            _lib.check(lib.wmf_posterior_draw_rows(*head, D, sigma, SEED, None, _ptr(X), *tail))
            out[f"{key}/draw{D}_sigma{sigma}"] = X.cpu().numpy()
        for tg in targets:
            T = tg.shape[1]
            mean, var = filled(n, T), filled(n, T)
            _lib.check(lib.wmf_posterior_score_rows(*head, _ptr(dev(tg, np.int32)), T, _ptr(mean), _ptr(var), *tail))
            out[f"{key}/mean{T}"], out[f"{key}/var{T}"] = mean.cpu().numpy(), var.cpu().numpy()
        out[f"{key}/failed_calls"] = fail.cpu().numpy()

    for name in explain_ref.case_names():
        c = explain_ref.inputs(name)
        run(c, f"explain/{name}", explain=c["targets"])
    identity, gated = posterior_ref.identity_case_names(), posterior_ref.gated_case_names()
    for name in foldin_ref.case_names():
        c = foldin_ref.inputs(name)
        run(c, f"foldin/{name}", foldin=True, draws=(1, 2) if name in identity else (), sigma=0.0)
        if name in gated:
            run(c, f"posterior/{name}", draws=DRAW_COUNTS, targets=[posterior_ref.targets_for(c, T) for T in TARGET_COUNTS])
    c = indefinite_case()
    run(c, "indefinite", explain=c["targets"], foldin=True, draws=DRAW_COUNTS, targets=[c["targets"]])
    np.savez(path, **out)
    print(f"{len(out)} arrays from {_lib.LIB_PATH} -> {path}")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    names = sorted(set(a.files) | set(b.files))
    bad = [k for k in names if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
           or a[k].tobytes() != b[k].tobytes()]
    for k in bad:
        print("DIFFERENT:", k)
    print(f"{len(names)} arrays, {len(bad)} differ")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
