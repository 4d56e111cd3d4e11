"""What the per-element GPU tests of the catalogue scans share (tests/test_gpu_recommend.py, tests/test_gpu_rank_positions.py,
tests/test_gpu_similar.py): the case tables of tests/test_gpu_serving.py, the plumbing to the C ABI, the factors and reference scores
of the two input classes (tests/serving_ref.py), the seen-row patterns and the order rule of the ROUNDED class."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import serving_ref as ref
from conftest import ROOT

WIDTHS = (1, 4, 5, 16, 63, 64, 65, 100, 128, 129, 144, 192, 193, 256, 257, 260)
LD_EXTRA = {5: 4, 64: 4, 100: 8, 129: 4, 257: 4, 260: 12}
CASES = [(f, b, 0) for f in WIDTHS for b in (0, 1) if f >= 2 or not b] + [(f, b, e) for f, e in LD_EXTRA.items() for b in (0, 1)]
case = pytest.mark.parametrize("f,bias,extra", CASES, ids=[f"f{f}-b{b}" + (f"-ld+{e}" if e else "") for f, b, e in CASES])
N_USERS, N_ITEMS = 40, 300
N_PATTERNS = 8


def _api():
    from recmodel_amd import _lib
    from recmodel_amd.engine import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _ld(f, extra=0):
    ld = _api()[1].wmf_ld_for(f) + extra
    assert ld % 4 == 0 and f <= ld <= 272
    return ld


def _constant(name, source):
    """The integer a #define of `source` (a path from the repository's root) gives `name`."""
    text = open(os.path.join(ROOT, source)).read()
    return int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", text).group(1))


@functools.lru_cache(maxsize=None)
def _host(f, cls):
    make = ref.exact_factors if cls == "exact" else ref.rounded_factors
    Uf, If = make(N_USERS, f, 10 * f + 1), make(N_ITEMS, f, 10 * f + 2)
    Uf.setflags(write=False)
    If.setflags(write=False)
    return Uf, If


@functools.lru_cache(maxsize=None)
def _scores(f, bias, cls):
    """Reference scores of every (user, item): int64 (EXACT) or float64 with its bound (ROUNDED).  Computed once, never written."""
    Uf, If = _host(f, cls)
    if cls == "exact":
        out = (ref.score_matrix_int(Uf, If, np.arange(N_USERS), np.arange(N_ITEMS), bias), None)
    else:
        uu, ii = np.repeat(np.arange(N_USERS), N_ITEMS), np.tile(np.arange(N_ITEMS), N_USERS)
        out = (ref.scores_f64(Uf, If, uu, ii, bias).reshape(N_USERS, N_ITEMS), ref.score_bound(Uf, If, uu, ii, bias).reshape(N_USERS, N_ITEMS))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _user_list(n=N_USERS):
    users = np.arange(n) % N_USERS
    if n > 9:
        users[9] = users[2]                                         # one user twice, with different seen rows (patterns 2 and 1)
    return users


def _seen_rows(rng, user_scores, n_items, shift):
    """One seen row per batch position, every pattern in turn: 0 nothing, 1 everything, 2 all but three, 3 one whole 16-item tile,
    4 exactly the 50 best-scoring items, 5 duplicated ids, 6 the last item (and a few more), 7 a random subset.  Ascending."""
    rows, everything = [], np.arange(n_items)
    for b, s in enumerate(user_scores):
        p = (b + shift) % N_PATTERNS
        if p == 0:
            row = everything[:0]
        elif p == 1:
            row = everything
        elif p == 2:
            row = np.delete(everything, rng.choice(n_items, min(3, n_items), replace=False))
        elif p == 3:
            t = int(rng.integers(0, (n_items + 15) // 16))
            row = everything[16 * t: 16 * t + 16]
        elif p == 4:
            row = np.sort(ref.stable_topn(s[:n_items], min(50, n_items)))
        elif p == 5:
            row = np.sort(np.repeat(rng.integers(0, n_items, 9), rng.integers(1, 4, 9)))
        elif p == 6:
            row = np.unique(np.append(rng.integers(0, n_items, 4), n_items - 1))
        else:
            row = np.flatnonzero(rng.random(n_items) < 0.3)
        rows.append(row.astype(np.int64))
    return rows


def _check_rounded_order(pos, ref_scores, bound, what):
    """The rule of tests/test_gpu_serving.py: positions are unique and the reference score of the k-th returned candidate is
    within B of the k-th best reference score (B of whichever of the two has the larger one).  Returns the worst ratio."""
    assert len(np.unique(pos)) == len(pos) and pos.min() >= 0 and pos.max() < len(ref_scores), what
    best = ref.stable_topn(ref_scores, len(pos))
    gap = np.abs(ref_scores[pos] - ref_scores[best])
    allowed = np.maximum(bound[pos], bound[best])
    ratio = float((gap / allowed).max())
    assert ratio <= 1.0, (what, ratio)
    return ratio
