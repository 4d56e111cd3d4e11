"""Host reference and cases of the short-row kernels (csrc/wmf_solve.hip: solve_pair_kernel, solve_low_kernel) and of the two pivoted
fallbacks they bounce rows to, for tests/test_gpu_low_rows.py: plain NumPy, no GPU.

    route_low, derive_widths   launch_low's dispatch restated: NCH, last1, the split-f16 tiles (X6), bstride and the kernel names
    lowrank, symmetric         g = V_u^T (I + D S)^-1 p, S = V_u V_u^T, and the symmetric form (I + E S E) y = E^-1 p, c = E y the
                               d >= 17 kernel eliminates, in any dtype; in float32 they are the yardstick E_lr32 of the gates
    x6_rows                    the row in float64 with the S tile the X6 kernels form (low_split8 restated): T_x6 of the gates
    yardsticks, gates          per row of a case: E_lr32 of its (family, degree class), T_x6, E_lu32 of the bounced rows, the gate
    build_case, pair_case, bounce_case, singular_case, launch_case   the rows the GPU tests solve; tests/test_low_ref_cpu.py asserts
                               the conditions on every build_case

The float64 reference of a row is iter_ref.solve_rows_ref; layouts, features() and row_errors() are iter_ref's.  The fixed side is
600 hand-made rows, one block of 100 per family (BLOCKS); a case's rows draw their columns from their family's block."""
import collections
import functools

import numpy as np

import iter_ref as R
from iter_ref import ld_for, is_split, features, row_errors, case_id  # noqa: F401  (re-exported for the tests)

M_FIXED = R.M_FIXED
HALF_ROW, WIDE_ROW = 5e-4, 1e-3                                      # tests/test_gpu_parity.py: rows of the other kernel families
MARGIN, GATE_CAP = 4.0, 2e-5
# Two kinds of rows are more than MARGIN times their yardstick away on the device (first run on an MI355X: 4 .. 8.7 and 3 .. 4.3
# up to f = 81), and the restated arithmetic of their kernels (emulate_low, emulate_pivoted below) shows the same on the host, so
# their margin is 1.5 x the worst restated figure over the cases (tests/test_low_ref_cpu.py asserts the figures):
#   rows of 17 .. 32 entries that are nearly one direction -- the aligned family, and every family at f <= 2 -- where the 2 x 2
#   block form multiplies by the explicit inverse of the leading tile and subtracts C - (B X) B^T: 10.95 x E_lr32 restated (11 below);
#   bounced rows: the pivoted kernels update the right-hand side in each of the f elimination steps (f roundings of every entry)
#   where LAPACK subtracts one accumulated sum: 15.2 x E_lu32 restated at f = 258, 6.5 in the median.
EMULATED_ALIGNED32, EMULATED_BOUNCED = 11.0, 15.2
MARGIN_ALIGNED32, MARGIN_BOUNCED = 1.5 * EMULATED_ALIGNED32, 1.5 * EMULATED_BOUNCED
COND_MAX = 100.0
CLASSES = ("pair", "low16", "low32")                                 # d <= 8, 9 .. 16, 17 .. 32

# ------------------------------------------------------------------------------------------------------------- the dispatch
Route = collections.namedtuple("Route", "pair low16 low32 fallback nch x6 last1 bstride split")


def route_low(f, bias, rolled=False):
    """What launch_low launches at width f for rows of d <= 8, 9 .. 16 and 17 .. 32, and the pivoted kernel of the bounced rows."""
    ld = ld_for(f)
    nch = (ld + 15) // 16
    last1 = f % 4 == 1 and ld == f + 3 and (ld // 4) % 4 == 1
    x6 = (ld % 32 == 0) if nch % 2 == 0 else (nch >= 3 and last1 and ld == 16 * (nch - 1) + 4)
    split = is_split(f, bias)
    bstride = 1
    if split:
        bstride = 3 if (rolled and f == 129 and x6 and nch == 9) else 2
    tf = "true" if x6 else "false"
    fallback = f"solve_general_kernel<{(f + 15) // 16}>" if f <= 144 else "solve_wide_lu_kernel"
    return Route(f"solve_pair_kernel<{nch}, {tf}>", f"solve_low_kernel<{nch}, 1, false, {tf}>", f"solve_low_kernel<{nch}, 2, true, {tf}>",
                 fallback, nch, x6, last1, bstride, split)


def low_names(route):
    return {route.pair, route.low16, route.low32}


def _key(f):
    return tuple((r.nch, r.x6, r.last1, r.split) for r in (route_low(f, 0), route_low(f, 1)))


def derive_widths():
    """Every f in 1 .. 260 at which NCH, X6, last1 or the split layout differs from f - 1, with f - 1; 1 .. 4 and 260, and 8
    (the pair kernel's longest row has as many entries as features)."""
    edges = {1, 2, 3, 4, 8, 260}
    for f in range(2, 261):
        if _key(f) != _key(f - 1):
            edges.update((f - 1, f))
    return sorted(edges)


WIDTHS = derive_widths()
CASES = [(f, b, False) for f in WIDTHS for b in (0, 1)] + [(129, 1, True)]


def every_shipped_name():
    return {n for f in range(1, 261) for b in (0, 1) for r in (False, True) for n in low_names(route_low(f, b, r))}


def degree_class(d):
    """0, 1, 2: the three short-row templates; 3: another kernel family (-1: no entries, the pair kernel writes the zero row)."""
    d = np.asarray(d)
    return np.where(d == 0, -1, np.where(d <= 8, 0, np.where(d <= 16, 1, np.where(d <= 32, 2, 3))))


# --------------------------------------------------------------------------------------------------------------- references
def lowrank(Vu, w, dtype=np.float32):
    """g = V_u^T (I + D S)^-1 (w + 1), S = V_u V_u^T, batched: Vu [B, d, f], w [B, d]; every operation in `dtype`."""
    Vu, w = np.asarray(Vu, dtype=dtype), np.asarray(w, dtype=dtype)
    S = Vu @ Vu.transpose(0, 2, 1)
    M = np.eye(Vu.shape[1], dtype=dtype) + w[:, :, None] * S
    c = np.linalg.solve(M, (w + dtype(1))[:, :, None])
    g = (Vu.transpose(0, 2, 1) @ c)[:, :, 0]
    assert g.dtype == dtype
    return g


def symmetric(Vu, w, dtype=np.float32):
    """The same row as c = E y, (I + E S E) y = E^-1 p, E = diag(sqrt(w)), a zero weight taken as 1e-30 (solve_low_kernel, BLK)."""
    Vu, w = np.asarray(Vu, dtype=dtype), np.asarray(w, dtype=dtype)
    wc = np.maximum(w, dtype(1e-30))
    e = np.sqrt(wc)
    S = Vu @ Vu.transpose(0, 2, 1)
    P = np.eye(Vu.shape[1], dtype=dtype) + e[:, :, None] * S * e[:, None, :]
    y = np.linalg.solve(P, ((w + dtype(1)) / e)[:, :, None])[:, :, 0]
    g = (Vu.transpose(0, 2, 1) @ (e * y)[:, :, None])[:, :, 0]
    assert g.dtype == dtype
    return g


def split8(v):
    """low_split8: the two f16 parts of 256 v (float32 in, float16 out); the subtraction is exact in float32."""
    s = (np.asarray(v, dtype=np.float32) * np.float32(256)).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def x6_tile(Vu, nsplit):
    """S [B, d, d] in float64 as the X6 kernels form it: (hi hi + hi lo + lo hi) / 65536 over the first nsplit features (whole
    32-feature chunks), the odd last piece exact."""
    hi, lo = split8(Vu[:, :, :nsplit])
    H, L = hi.astype(np.float64), lo.astype(np.float64)
    T = np.asarray(Vu[:, :, nsplit:], dtype=np.float64)
    Ht, Lt = H.transpose(0, 2, 1), L.transpose(0, 2, 1)
    return (H @ Ht + H @ Lt + L @ Ht) / 65536.0 + T @ T.transpose(0, 2, 1)


def x6_rows(Vu, w, nsplit):
    """The rows in float64 with the X6 tile in place of S."""
    V64, w = np.asarray(Vu, dtype=np.float64), np.asarray(w, dtype=np.float64)
    M = np.eye(V64.shape[1]) + w[:, :, None] * x6_tile(Vu, nsplit)
    c = np.linalg.solve(M, (w + 1)[:, :, None])
    return (V64.transpose(0, 2, 1) @ c)[:, :, 0]


def nsplit_of(route, f):
    """Features the X6 kernels take through the f16 split (0: not an X6 kernel)."""
    if not route.x6:
        return 0
    return f if route.nch % 2 == 0 else f - 1


def cond_sym(Vu, w):
    """cond_2(I + E S E) in float64, batched."""
    V64, w = np.asarray(Vu, dtype=np.float64), np.maximum(np.asarray(w, dtype=np.float64), 0.0)
    e = np.sqrt(w)
    ev = np.linalg.eigvalsh(np.eye(V64.shape[1]) + e[:, :, None] * (V64 @ V64.transpose(0, 2, 1)) * e[:, None, :])
    return ev[:, -1] / ev[:, 0]


# -------------------------------------------------------------------------------------------------------------------- cases
# family: (first row of its block of 100, row norm)
BLOCKS = {"near": (0, 0.03), "balanced": (100, 0.3), "stiff": (200, 0.9), "aligned": (300, 0.03), "tiny3": (400, 1e-3), "tiny4": (500, 1e-4)}
FAMILIES = tuple(BLOCKS)
TAMED = ("stiff", "aligned")                                         # weights halved until cond(I + E S E) <= COND_MAX
ZERO_BIAS, SOME_BIAS = 1, 2                                          # columns of every block whose bias is 0 and 1/8
ROLLED_BORDER = 2.0 ** -17
REPS = 3


def _fixed_side(f, bias, rolled, rng, unit_row=None):
    """U float32 [600, f] and bias float32 [600] (multiples of 2^-6) or None.  Blocks of 100 rows with Gaussian directions and the
    block's norm (1 +- 0.1); the aligned block is v_0 + 1e-3 noise, renormalised.  rolled: the border feature is one number.
    unit_row: that row is e_1 (singular_case)."""
    U = rng.standard_normal((M_FIXED, f))
    if f <= 2:
        # up to 33 entries in one or two dimensions: with features of both signs V_u^T c cancels and NO float32 evaluation of the
        # row stays under GATE_CAP (measured on the host: 7e-5 .. 5e-4); with features of one sign nothing cancels
        U = np.abs(U)
    off = BLOCKS["aligned"][0]
    main = U[off] / np.linalg.norm(U[off])
    noise = rng.standard_normal((100, f))
    U[off: off + 100] = main + 1e-3 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    norms = np.concatenate([np.full(100, nrm) for _, nrm in BLOCKS.values()]) * (1 + 0.1 * (2 * rng.random(M_FIXED) - 1))
    if rolled:
        body = U[:, :f - 1]
        body *= (np.sqrt(norms ** 2 - ROLLED_BORDER ** 2) / np.linalg.norm(body, axis=1))[:, None]
        U = np.concatenate([body, np.full((M_FIXED, 1), ROLLED_BORDER)], axis=1)
    else:
        U *= (norms / np.linalg.norm(U, axis=1))[:, None]
    if unit_row is not None:
        U[unit_row] = 0.0
        U[unit_row, 0] = 1.0
    b = None
    if bias:
        b = (rng.integers(-16, 17, M_FIXED) / 64.0).astype(np.float32)
        b[ZERO_BIAS::100] = 0.0
        b[SOME_BIAS::100] = 0.125
        if unit_row is not None:
            b[unit_row] = 0.25
    return U.astype(np.float32), b


def _base_weights(rng, fam, d):
    if fam == "near":
        return 10 * np.log(1 + rng.integers(1, 8, d))
    if fam == "balanced":
        return 10 * (0.5 + rng.random(d))
    if fam == "stiff":
        return 1e6 * (0.5 + 0.5 * rng.random(d))
    if fam == "aligned":
        return 1e3 * (0.5 + rng.random(d))
    return 1e6 * (0.75 + 0.5 * rng.random(d))                        # tiny3, tiny4


def _effective(w, b, cols):
    """(stored values float32, the weights the kernels see: float32(value - bias))."""
    bb = b[cols] if b is not None else np.zeros(len(cols), dtype=np.float32)
    values = (np.asarray(w, dtype=np.float64) + bb.astype(np.float64)).astype(np.float32)
    return values, values - bb


def cond_full(Vu, w):
    """cond_2(I + V_u^T D V_u), the f x f matrix, in float64 (w >= 0): with fewer entries than features it keeps the eigenvalue 1."""
    V64, w = np.asarray(Vu, dtype=np.float64), np.maximum(np.asarray(w, dtype=np.float64), 0.0)
    e = np.sqrt(w)
    ev = np.linalg.eigvalsh(np.eye(V64.shape[1]) + e[:, :, None] * (V64 @ V64.transpose(0, 2, 1)) * e[:, None, :])
    lo = np.minimum(ev[:, 0], 1.0) if V64.shape[1] < V64.shape[2] else ev[:, 0]
    return ev[:, -1] / lo


def _tame(U, b, cols, w):
    """Halve the row's weights until cond_2(I + E S E) <= COND_MAX in float64, on the weights the kernels see.  A row of 33
    entries is no short row: the kernels that take it eliminate f x f, where float32 is good to 6e-8 cond_2(A_u) -- for it the
    rule is applied to that matrix (its gate is those kernels' 5e-4 / 1e-3, and weights of 1e6 on cond(A_u) = 1e6 miss it in
    LAPACK's float32 as well)."""
    Vu = U[cols][None]
    cond = cond_sym if len(cols) <= 32 else cond_full
    k = 0
    while cond(Vu, _effective(w / 2.0 ** k, b, cols)[1][None])[0] > COND_MAX:
        k += 1
    return w / 2.0 ** k, k


class Case(R.Case):
    """iter_ref.Case with, per row, the tag of a special row ("" otherwise) and how often its weights were halved."""

    def __init__(self, *args, tags, halved):
        super().__init__(*args)
        self.tags, self.halved = tags, halved
        self.route = route_low(self.f, self.bias, self.rolled)
        self.cls = degree_class(self.degree)

    def inputs(self):
        """(U float32 [m, f], effective weights float32 [nnz]) as the kernels read them."""
        if getattr(self, "_inputs", None) is None:
            self._inputs = self._read_inputs()
        return self._inputs

    def ref(self):
        """iter_ref.solve_rows_ref; the exactly singular rows (tag "unit") have no solution and stay 0."""
        unit = self.tags == "unit"
        if not unit.any():
            return super().ref()
        keep = np.flatnonzero(~unit)
        out = np.zeros((self.n, self.ld))
        out[keep] = self.subset(keep).ref()
        return out

    def _read_inputs(self):
        U, b = features(np.asarray(self.V), self.side, self.f, self.rolled)
        if b is None and self.bias_fixed is not None:
            b = self.bias_fixed
        w = self.values if b is None else self.values - b[self.indices]
        return U, w

    def gather(self, rows):
        """(Vu [B, d, f], w [B, d]) of rows of one degree."""
        U, w = self.inputs()
        at = self.indptr[rows][:, None] + np.arange(self.degree[rows[0]])[None, :]
        return U[self.indices[at]], w[at]

    def negative(self):
        w = self.inputs()[1]
        neg = np.zeros(self.n, dtype=bool)
        np.logical_or.at(neg, np.repeat(np.arange(self.n), self.degree), ~(w >= 0))
        return neg

    def pairs(self):
        """The pairs solve_pair_kernel makes: the rows of at most 8 entries in row order, two by two (-1: no partner)."""
        short = np.flatnonzero(self.degree <= 8)
        if len(short) % 2:
            short = np.concatenate([short, [-1]])
        return short.reshape(-1, 2)

    def bounced(self):
        """Rows the short-row kernels hand to the pivoted fallback: a negative effective weight, or a pair partner's."""
        neg = self.negative() & (self.degree <= 32)
        out = neg.copy()
        for a, b in self.pairs():
            if b >= 0 and (neg[a] or neg[b]):
                out[a] = out[b] = True
        return out

    def subset(self, rows):
        deg = self.degree[rows]
        indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        take = np.concatenate([np.arange(self.indptr[u], self.indptr[u + 1]) for u in rows] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        return Case(self.f, self.bias, self.rolled, self.V, self.side, self.bias_fixed, indptr, self.indices[take].copy(),
                    self.values[take].copy(), self.family[rows], {}, tags=self.tags[rows], halved=self.halved[rows])


def _make_row(rng, U, b, fam, d, tag, unit_row=None):
    """(columns, stored values, halvings) of one row.  Tags: zero_first / zero_mid / zero_last (a stored zero: w = 0, p = 1),
    eqbias (value == bias != 0), dup (a column twice), ends (columns 0 and m - 1), neg (a negative value), negbias (0 < value < bias),
    unit (the one entry e_1 with w = -1)."""
    if tag == "unit":
        cols = np.array([unit_row], dtype=np.int32)
        return cols, _effective(np.array([-1.0]), b, cols)[0], 0
    off = BLOCKS[fam][0]
    cols = (rng.choice(97, d, replace=False) + 3 + off).astype(np.int32)
    w = _base_weights(rng, fam, d)
    pos = {"zero_first": 0, "zero_last": d - 1}.get(tag, d // 2)
    if tag == "dup":
        cols[d // 3] = cols[d - 1]
    if tag == "ends":
        cols[0], cols[-1] = 0, M_FIXED - 1
    if tag in ("zero_first", "zero_mid", "zero_last"):
        cols[pos], w[pos] = off + ZERO_BIAS, 0.0
    if tag == "eqbias":
        cols[pos], w[pos] = off + SOME_BIAS, 0.0
    if tag == "negbias":
        cols[pos], w[pos] = off + SOME_BIAS, -0.0625
    if tag == "neg":
        w[pos] = -5.0
    k = 0
    if fam in TAMED:
        w, k = _tame(U, b, cols, w)
    return cols, _effective(w, b, cols)[0], k


def _assemble(f, bias, rolled, seed, plan, unit_row=None):
    """plan: [(family, d, tag)]; d = 0 is an empty row."""
    rng = np.random.default_rng(seed)
    U, b = _fixed_side(f, bias, rolled, rng, unit_row)
    V, side, bias_fixed = R._layout(f, bias, rolled, U, b)
    U = features(V, side, f, rolled)[0]                              # (the rolled layout moved body values by an ulp)
    cols_all, vals_all, halved = [], [], []
    for fam, d, tag in plan:
        if d == 0:
            cols, vals, k = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), 0
        else:
            cols, vals, k = _make_row(rng, U, b, fam, d, tag, unit_row)
        cols_all.append(cols)
        vals_all.append(vals)
        halved.append(k)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols_all])]).astype(np.int64)
    fams = np.array([fam if d else "" for fam, d, _ in plan], dtype=object)
    tags = np.array([tag or "" for _, _, tag in plan], dtype=object)
    return Case(f, bias, rolled, V, side, bias_fixed, indptr, np.concatenate(cols_all).astype(np.int32),
                np.concatenate(vals_all).astype(np.float32), fams, {}, tags=tags, halved=np.array(halved))


def families_at(f, d):
    """Rows with more entries than features (the widths below 32) come from the first two families only."""
    return FAMILIES[:2] if d > f else FAMILIES


def case_plan(f, bias):
    """Row order of a build_case.  Front: an empty row, a row whose entries start `indices`, three (negative row, partner) pairs,
    negative rows of 12 and 24 entries, an empty row between two full pairs.  Middle, shuffled: every family at every degree
    1 .. 33, REPS rows each, empty rows, the structure rows.  Back: a row whose entries end `indices`, an empty row."""
    front = [("", 0, None), ("near", 7, "straddle")]
    for k in range(3):
        front += [("near", 5, "negbias" if bias and k == 1 else "neg"), ("near", 4 + k, "partner")]
    front += [("near", d, "negbias" if bias and k == 1 else "neg") for d in (12, 24) for k in range(3)]
    front += [("balanced", 8, "full"), ("balanced", 8, "full"), ("", 0, None), ("balanced", 8, "full"), ("balanced", 8, "full"), ("balanced", 8, "full")]
    mid = [(fam, d, None) for d in range(1, 34) for fam in families_at(f, d) for _ in range(REPS)]
    mid += [("", 0, None)] * REPS
    for k, d in enumerate((6, 12, 24)):
        fam = ("near", "balanced")[k % 2]
        mid += [(fam, d, t) for t in ("zero_first", "zero_mid", "zero_last", "eqbias", "dup", "ends")]
    rng = np.random.default_rng(100 + f)
    mid = [mid[i] for i in rng.permutation(len(mid))]
    return front + mid + [("near", 9, "straddle"), ("", 0, None)]


STRUCTURE_TAGS = ("zero_first", "zero_mid", "zero_last", "eqbias", "dup", "ends")   # ("straddle" and "full" rows are ordinary rows of their family)


def _relabel(case):
    """The special rows are gated as families of their own: "structure" and "negative" (partners of bounced pairs keep theirs)."""
    fam = case.family.copy()
    fam[np.isin(case.tags, STRUCTURE_TAGS)] = "structure"
    fam[np.isin(case.tags, ("neg", "negbias", "partner", "unit"))] = "negative"
    case.family = fam
    return case


@functools.lru_cache(maxsize=None)
def build_case(f, bias, rolled=False):
    return _relabel(_assemble(f, bias, rolled, 15000 + 4 * f + 2 * int(bias) + int(rolled), case_plan(f, bias)))


PAIR_WIDTHS = ((50, 0, False), (64, 0, False), (81, 1, False), (129, 1, True))   # plain, X6, split, rolled


@functools.lru_cache(maxsize=None)
def pair_case(f, bias, rolled=False):
    """All 81 ordered pairs (dA, dB) in 0 .. 8 as consecutive rows -- every row has at most 8 entries, so the plan's order is the
    row order -- and a last row without a partner; behind them rows of 9 .. 32 entries in random order."""
    rng = np.random.default_rng(7 + f)
    plan = []
    for k in rng.permutation(81):
        plan += [(("balanced", "near")[int(k) % 2], int(k) // 9, None), (("balanced", "stiff")[int(k) % 3 == 0], int(k) % 9, None)]
    plan.append(("balanced", 5, None))
    plan += [(("balanced", "near", "stiff")[int(d) % 3], int(d), None) for d in rng.permutation(np.arange(9, 33))]
    return _relabel(_assemble(f, bias, rolled, 21000 + 4 * f + 2 * int(bias) + int(rolled), plan))


BOUNCE_WIDTHS = ((16, 0, False, 260), (17, 1, False, 40), (50, 1, False, 40), (129, 1, False, 270), (129, 1, True, 40), (200, 0, False, 70),
                 (200, 1, False, 40))


@functools.lru_cache(maxsize=None)
def bounce_case(f, bias, rolled, count):
    """`count` bounced rows and more: negative rows as row A and as row B of a pair, of 12 and of 24 entries, through a negative
    value and (bias) through 0 < value < bias; their partners; a few ordinary rows in between."""
    kinds = ["neg", "negbias"] if bias else ["neg"]
    plan = []
    for i in range((count + 3) // 4):                                # four bounced rows per round
        tag = kinds[(i // 2) % len(kinds)]
        if i % 2 == 0:
            plan += [("near", 5, tag), ("near", 3 + i % 5, "partner")]               # row A negative
        else:
            plan += [("balanced", 2 + i % 7, "partner"), ("near", 6, tag)]           # row B negative
        plan += [("near", 12, tag), ("near", 24, tag), ("balanced", 4, None), ("balanced", 7, None), ("near", 20, None)]
    return _relabel(_assemble(f, bias, rolled, 23000 + 4 * f + 2 * int(bias) + int(rolled), plan))


SINGULAR_WIDTHS = ((16, 0, 3), (129, 0, 2), (129, 1, 3), (200, 0, 2), (200, 1, 1))
UNIT_ROW = 250


@functools.lru_cache(maxsize=None)
def singular_case(f, bias, k):
    """k rows whose one entry is e_1 with effective weight -1 (A = I - e_1 e_1^T: pivot column 0 is exactly zero) among ordinary
    rows; the singular rows are paired with each other and with ordinary rows."""
    plan = [("balanced", 6, None), ("near", 20, None)]
    for i in range(k):
        plan += [("near", 1, "unit"), ("near", 3 + i, "partner"), ("balanced", 12, None)]
    plan += [("near", 5, "neg"), ("balanced", 30, None), ("near", 2, None)]
    return _relabel(_assemble(f, bias, False, 25000 + 4 * f + 2 * int(bias), plan, unit_row=UNIT_ROW))


def launch_case(f, bias, rolled=False):
    """The four rows of the launched-kernels test: 3, 12 and 24 entries and a negative row of 5."""
    plan = [("balanced", 3, None), ("balanced", 12, None), ("balanced", 24, None), ("near", 5, "neg")]
    return _relabel(_assemble(f, bias, rolled, 27000 + 4 * f + 2 * int(bias) + int(rolled), plan))


# ------------------------------------------------------------------------------------------------------ yardsticks and gates
def yardsticks(case, ref=None, orders=1):
    """Per row, against the float64 reference: e_lr (NumPy float32 d x d, the worse of the two forms for d >= 17; NaN for a row
    with a negative weight or more than 32 entries), t_x6, cond (of I + E S E).  orders > 1: the float32 forms are also run with
    the features and the entries in `orders - 1` other orders and the worst counts -- a one-row class has no other sample of the order of the sums."""
    ref = case.ref() if ref is None else ref
    f, n = case.f, case.n
    e_lr, t_x6, cond = np.full(n, np.nan), np.zeros(n), np.ones(n)
    neg = case.negative()
    nsplit = nsplit_of(case.route, f)
    for d in np.unique(case.degree):
        rows = np.flatnonzero((case.degree == d) & ~neg)
        if d == 0 or d > 32 or not len(rows):
            continue
        Vu, w = case.gather(rows)
        want = ref[rows, :f]
        err = np.zeros(len(rows))
        for k in range(orders):
            rng = np.random.default_rng(k)
            perm, ent = (np.arange(f), np.arange(d)) if k == 0 else (rng.permutation(f), rng.permutation(d))
            Vp, wp = np.ascontiguousarray(Vu[:, ent][:, :, perm]), np.ascontiguousarray(w[:, ent])
            err = np.maximum(err, row_errors(lowrank(Vp, wp), want[:, perm]))
            if d >= 17:
                err = np.maximum(err, row_errors(symmetric(Vp, wp), want[:, perm]))
        e_lr[rows] = err
        if nsplit:
            t_x6[rows] = row_errors(x6_rows(Vu, w, nsplit), want)
        cond[rows] = cond_sym(Vu, w)
    return {"e_lr": e_lr, "t_x6": t_x6, "cond": cond}


def ref_lowrank64(case):
    """The rows of at most 33 entries by the d x d form in float64 (tests/test_low_ref_cpu.py: equal to iter_ref.solve_rows_ref to
    1e-12); the others, and the exactly singular ones, stay 0."""
    out = np.zeros((case.n, case.ld))
    for d in np.unique(case.degree):
        rows = np.flatnonzero((case.degree == d) & (case.tags != "unit"))
        if 0 < d <= 33 and len(rows):
            Vu, w = case.gather(rows)
            out[rows, :case.f] = lowrank(Vu, w, np.float64)
    return out


def lu32_errors(case, rows, ref):
    """Row errors of iter_ref.solve_rows_f32 (f x f, LAPACK) on `rows`."""
    if not len(rows):
        return np.zeros(0)
    sub = case.subset(rows)
    return row_errors(sub.f32()[:, :case.f], ref[rows, :case.f])


def margin_of(case, fam, cls):
    """MARGIN, or the widened margin of a nearly one-directional row in the block form (see MARGIN_ALIGNED32)."""
    return MARGIN_ALIGNED32 if cls == "low32" and (fam == "aligned" or case.f <= 2) else MARGIN


def gates(case, ref=None, ys=None, orders=1):
    """Per row (gate, kind): kind is "pair" / "low16" / "low32" (margin_of x E_lr32 of the row's (family, class) + its T_x6), "bounced"
    (MARGIN_BOUNCED x E_lu32 of the case), "other" (the other kernel families' tolerance) or "empty" (exactly 0).  Also the yardsticks used."""
    ref = case.ref() if ref is None else ref
    ys = yardsticks(case, ref, orders) if ys is None else ys
    bounced = case.bounced() & (case.tags != "unit")
    gate, kind = np.zeros(case.n), np.empty(case.n, dtype=object)
    kind[:] = "other"
    gate[:] = WIDE_ROW if case.f > 144 else HALF_ROW
    kind[case.degree == 0] = "empty"
    gate[case.degree == 0] = 0.0
    kind[case.tags == "unit"] = "singular"                           # reported through fail_count, the row is exactly 0
    gate[case.tags == "unit"] = 0.0
    E = {}
    solved = ~bounced & (case.cls >= 0) & (case.cls <= 2) & (case.tags != "unit")
    for fam in sorted(set(case.family[solved])):
        for c in range(3):
            sel = solved & (case.family == fam) & (case.cls == c)
            if sel.any():
                E[(fam, CLASSES[c])] = float(ys["e_lr"][sel].max())
                gate[sel] = margin_of(case, fam, CLASSES[c]) * E[(fam, CLASSES[c])] + ys["t_x6"][sel]
                kind[sel] = CLASSES[c]
    rows = np.flatnonzero(bounced & (case.degree > 0))
    if len(rows):
        E["bounced"] = float(lu32_errors(case, rows, ref).max())
        gate[rows] = MARGIN_BOUNCED * E["bounced"]
        kind[rows] = "bounced"
    return gate, kind, E, ys


# ------------------------------------------------------------------------------------------- the kernels' arithmetic restated
# NumPy float32 restatements of the eliminations the kernels run, for the families whose device error is more than MARGIN times
# the yardstick: they show whether that is the order of the kernel's operations or a wrong kernel (tests/test_low_ref_cpu.py).
def _gj_solve32(m, p, steps):
    """gj_sweep: Gauss-Jordan without pivoting on [B, n, n], pivot rows left un-normalised, p scaled by 1 / piv at the end."""
    m, p = m.copy(), p.copy()
    dsc = np.ones_like(p)
    for K in range(steps):
        inv = np.float32(1) / m[:, K, K]
        nf = -m[:, :, K] * inv[:, None]
        nf[:, K] = 0
        m += nf[:, :, None] * m[:, K, None, :]
        p += nf * p[:, K, None]
        dsc[:, K] = inv
    return p * dsc


def _gj_inverse32(a):
    """gj_inv_sweep: in-place Gauss-Jordan inverse of [B, 16, 16], un-normalised sweep."""
    a = a.copy()
    dsc = np.ones(a.shape[:2], dtype=np.float32)
    for K in range(a.shape[1]):
        inv = np.float32(1) / a[:, K, K]
        nf = -a[:, :, K] * inv[:, None]
        nf[:, K] = 0
        a[:, :, K] = 0
        a[:, K, K] = 1
        a += nf[:, :, None] * a[:, K, None, :]
        dsc[:, K] = inv
    return a * dsc[:, :, None]


def emulate_low(Vu, w):
    """solve_low_kernel's arithmetic on rows of one degree in NumPy float32: d <= 16 the sweep on I + D S, d >= 17 the symmetric
    2 x 2 block elimination (X = A^-1 explicitly, S' = C - (B X) B^T, two tile solves).  Sums in NumPy's order, not the MFMAs'."""
    Vu, w = np.asarray(Vu, dtype=np.float32), np.asarray(w, dtype=np.float32)
    B, d, f = Vu.shape
    one = np.float32(1)
    S = Vu @ Vu.transpose(0, 2, 1)
    p = w + one
    if d <= 16:
        c = _gj_solve32(np.eye(d, dtype=np.float32) + w[:, :, None] * S, p, d)
    else:
        n = 32
        Sp = np.zeros((B, n, n), dtype=np.float32)
        Sp[:, :d, :d] = S
        wp, pp = np.zeros((B, n), dtype=np.float32), np.zeros((B, n), dtype=np.float32)
        wp[:, :d], pp[:, :d] = w, p
        wc = np.maximum(wp, np.float32(1e-30))
        e = np.sqrt(wc)
        P = np.eye(n, dtype=np.float32) + (e[:, :, None] * Sp) * e[:, None, :]
        t = pp * (one / e)
        PA, PU, PB, PC = P[:, :16, :16], P[:, :16, 16:], P[:, 16:, :16], P[:, 16:, 16:]
        X = _gj_inverse32(PA)
        T = PB @ X
        SC = PC - T @ PB.transpose(0, 2, 1)
        tB = t[:, 16:] - (T @ t[:, :16, None])[:, :, 0]
        yB = _gj_solve32(SC, tB, 4 * ((d - 16 + 3) // 4))
        z = t[:, :16] - (PU @ yB[:, :, None])[:, :, 0]
        yA = (X @ z[:, :, None])[:, :, 0]
        c = (e * np.concatenate([yA, yB], axis=1))[:, :d]
    g = (Vu.transpose(0, 2, 1) @ c[:, :, None])[:, :, 0]
    assert g.dtype == np.float32
    return g


def emulate_pivoted(Vu, w):
    """solve_general_kernel / solve_wide_lu_kernel on rows of one degree in NumPy float32: B = I + sum_j w_j v_j v_j^T entry by
    entry, right-looking LU that updates the right-hand side in every step, column-oriented back substitution.  Rows whose
    pivot search would swap are not restated (asserted: none among the cases' bounced rows, which are near the identity)."""
    Vu, w = np.asarray(Vu, dtype=np.float32), np.asarray(w, dtype=np.float32)
    n, d, f = Vu.shape
    A = np.broadcast_to(np.eye(f, dtype=np.float32), (n, f, f)).copy()
    rhs = np.zeros((n, f), dtype=np.float32)
    for j in range(d):
        A += (w[:, j, None] * Vu[:, j])[:, :, None] * Vu[:, j, None, :]
        rhs += (w[:, j, None] + np.float32(1)) * Vu[:, j]
    for k in range(f - 1):
        assert (np.abs(A[:, k + 1:, k]).max(axis=1) < np.abs(A[:, k, k])).all(), "a row swap"
        l = A[:, k + 1:, k] * (np.float32(1) / A[:, k, k])[:, None]
        A[:, k + 1:, k + 1:] -= l[:, :, None] * A[:, k, None, k + 1:]
        rhs[:, k + 1:] -= l * rhs[:, k, None]
    for k in range(f - 1, -1, -1):
        xk = rhs[:, k] / A[:, k, k]
        rhs[:, :k] -= A[:, :k, k] * xk[:, None]
        rhs[:, k] = xk
    assert rhs.dtype == np.float32
    return rhs


def emulated_errors(case, ref, rows, pivoted=False):
    """Row errors of the restated kernel arithmetic on `rows`."""
    out = np.zeros(len(rows))
    for d in np.unique(case.degree[rows]):
        sel = np.flatnonzero(case.degree[rows] == d)
        Vu, w = case.gather(rows[sel])
        g = emulate_pivoted(Vu, w) if pivoted else emulate_low(Vu, w)
        out[sel] = row_errors(g, ref[rows[sel], :case.f])
    return out
