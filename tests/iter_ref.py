"""Host reference of the float32 matrix-free iteration (csrc/wmf_iter.hip) for tests/test_gpu_iter_rows.py: plain NumPy, no GPU.

    solve_rows_ref    float64 g_u = (I + V_u^T D V_u)^-1 V_u^T (w + 1) from exactly the float32 arrays a test uploads
    solve_rows_f32    the same rows in NumPy float32 (A formed in float32, LAPACK's float32 solve): the yardstick E32 of the gates
    policy            the decision code of solve_iter_kernel restated in float64: which path a row takes, after how many
                      applications of E
    route, iter_dmax  wmf_launch_iter / wmf_iter_dmax of the shipped build restated
    build_case, pipeline_case, minor_case   the rows the GPU tests solve; tests/test_iter_ref_cpu.py asserts on every one of them
                      the margins that make policy()'s float64 prediction the float32 kernel's path

Layouts (include/wmf_hip.h).  Plain: V is [m, ld] with zero padding columns, bias_fixed float[m] or None.  Split (bias models at
f = 17, 33, 65, 81, 97, 129, ld = f + 3): V is the packed body [m, f - 1], side float[m, 2] = {last feature, bias}.  Rolled
(f = 129 with biases, WMF_SOLVE_ROLLED): the split layout whose border feature is one number for every row and whose body
carries the 32 bits of the row's bias in the last mantissa bit of positions 8 j, 8 j + 1 (bits 2 j, 2 j + 1).  g is [n, ld]: the
body coordinates first, the border coordinate at f - 1, zero padding -- for the reference the row is the f-vector {body, border}
whatever the coordinates are called."""
import functools

import numpy as np

TAU_NEUMANN, KAPPA_MAX, KMAX, EPS = 0.8, 4.0, 20, 1.2e-7           # IT_DEFAULTS of csrc/wmf_iter.hip
SPLIT_WIDTHS = (17, 33, 65, 81, 97, 129)                            # wmf_dw_border(f): f = 16 m + 1 <= 144, m % 4 != 3
M_FIXED, BLOCK = 600, 300
ROW_NORM = 0.03
EDGES = (33, 34, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256)
SOLVED = ("neumann", "switch", "chebyshev")


# ------------------------------------------------------------------------------------------------------------- the dispatch
def ld_for(f):
    return (f + 3) & ~3


def is_split(f, bias):
    return bool(bias) and f in SPLIT_WIDTHS


def ldv_of(f, bias):
    return f - 1 if is_split(f, bias) else ld_for(f)


def _name(nw, fpl, ns, split, full, occ, dma=False, lsb=False):
    tf = ("false", "true")
    return f"solve_iter_kernel<{nw}, {fpl}, {ns}, {tf[split]}, {tf[full]}, {occ}, {tf[dma]}, {tf[lsb]}>"


def route(f, bias, rolled=False):
    """The iteration kernels one solve launches at width f (names as the library's profile records them), in launch order."""
    split, ldv = is_split(f, bias), ldv_of(f, bias)
    lsb = bool(rolled) and split and f == 129
    if ldv < 65 or ldv > 320:
        return ()
    if ldv == 128:
        return (_name(2, 8, 16, split, True, 2, False, lsb), _name(4, 8, 8, split, True, 2, True, lsb))
    if ldv < 128:
        return (_name(4, 8, 9, split, False, 2 if split else 3),)
    if ldv <= 192:
        return (_name(8, 12, 8, False, ldv == 192, 2),)
    if ldv <= 256:
        return (_name(8, 16, 8, False, ldv == 256, 2),)
    return (_name(8, 20, 6, False, False, 2),)


def iter_dmax(f, bias):
    """Rows of 33 .. iter_dmax entries are the iteration's candidates (0: none at this width)."""
    ldv = ldv_of(f, bias)
    if ldv < 65:
        return 0
    if ldv == 128:
        return 128
    if ldv < 128:
        return 144
    return 256 if ldv <= 256 else 192


def grid_cap(f, bias):
    """Workgroups of the (first) iteration kernel's launch at most: four rounds of what the chip holds."""
    ldv = ldv_of(f, bias)
    if ldv == 128:
        return 4096
    if ldv < 128:
        return 2048 if is_split(f, bias) else 3072
    return 1024


def entries_per_slot(f, bias):
    """4 NW of the kernel that takes the candidates first."""
    ldv = ldv_of(f, bias)
    return 8 if ldv == 128 else 16 if ldv < 128 else 32


def derive_widths():
    edges = {125, 127, 189, 253, 260}
    for f in range(2, 261):
        if any(route(f, b) != route(f - 1, b) or iter_dmax(f, b) != iter_dmax(f - 1, b) for b in (0, 1)):
            edges.update((f - 1, f))
    return sorted(edges)


WIDTHS = derive_widths()


# --------------------------------------------------------------------------------------------------------------- references
def rolled_bias(V):
    """The 32 bits the rolled layout keeps in the last mantissa bits of body positions 8 j, 8 j + 1, as float32[m]."""
    bits = np.ascontiguousarray(V[:, :128]).view(np.uint32) & np.uint32(1)
    word = np.zeros(V.shape[0], dtype=np.uint32)
    for j in range(16):
        word |= (bits[:, 8 * j] << np.uint32(2 * j)) | (bits[:, 8 * j + 1] << np.uint32(2 * j + 1))
    return word.view(np.float32)


def features(V, side, f, rolled=False):
    """(U float32 [m, f], bias float32 [m] or None): the rows' f features and the fixed side's bias as the kernels read them."""
    if side is None:
        return V[:, :f], None
    side = np.asarray(side).reshape(-1, 2)
    assert V.shape[1] == f - 1
    if rolled:
        border = np.full(V.shape[0], side[0, 0], dtype=np.float32)   # (the kernels read side[0] only)
        return np.concatenate([V, border[:, None]], axis=1), rolled_bias(V)
    return np.concatenate([V, side[:, :1]], axis=1), side[:, 1]


def _row_inputs(V, side, bias_fixed, indptr, indices, values, f, rolled):
    U, bias = features(np.asarray(V, dtype=np.float32), side, f, rolled)
    if bias is None and bias_fixed is not None:
        bias = np.asarray(bias_fixed, dtype=np.float32)
    values = np.asarray(values, dtype=np.float32)
    for u in range(len(indptr) - 1):
        idx = np.asarray(indices[indptr[u]: indptr[u + 1]], dtype=np.int64)
        w = values[indptr[u]: indptr[u + 1]]
        if bias is not None:
            w = w - bias[idx]                                        # float32, as the kernels subtract it
        yield u, U[idx], w


def solve_rows_ref(V, side, bias_fixed, indptr, indices, values, f, rolled=False):
    """float64 g [n, ld_for(f)]; stored zeros count, duplicates are separate entries, an empty row gives 0."""
    g = np.zeros((len(indptr) - 1, ld_for(f)))
    for u, Vu, w in _row_inputs(V, side, bias_fixed, indptr, indices, values, f, rolled):
        if len(w):
            Vu, w = Vu.astype(np.float64), w.astype(np.float64)
            g[u, :f] = np.linalg.solve(np.eye(f) + Vu.T @ (Vu * w[:, None]), Vu.T @ (w + 1))
    return g


def solve_rows_f32(V, side, bias_fixed, indptr, indices, values, f, rolled=False):
    """The same rows with every operation in float32."""
    g = np.zeros((len(indptr) - 1, ld_for(f)), dtype=np.float32)
    for u, Vu, w in _row_inputs(V, side, bias_fixed, indptr, indices, values, f, rolled):
        if len(w):
            A = np.eye(f, dtype=np.float32) + Vu.T @ (Vu * w[:, None])
            b = Vu.T @ (w + np.float32(1))
            assert A.dtype == np.float32 and b.dtype == np.float32
            g[u, :f] = np.linalg.solve(A, b)
    assert g.dtype == np.float32
    return g


def row_errors(got, ref):
    """||got_u - ref_u|| / ||ref_u|| per row; 0 for a pair of zero rows, inf for a non-zero row against zero."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    num, den = np.linalg.norm(got - ref, axis=1), np.linalg.norm(ref, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))


# ------------------------------------------------------------------------------------------------------------------- policy
def policy_detail(Vu, w, cheb=True, tau_neumann=TAU_NEUMANN):
    """solve_iter_kernel's decisions on one row in float64.  Vu [d, f] (border feature included), w [d] the weights after the
    bias.  cheb=False: the two-wave stage, which has no Chebyshev recurrence and hands on what needs it."""
    Vu, w = np.asarray(Vu, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n2 = (Vu * Vu).sum(axis=1)
    tp, tn = float((np.maximum(w, 0) * n2).sum()), float((np.maximum(-w, 0) * n2).sum())
    b = Vu.T @ (w + 1)
    nb = float(b @ b)
    tau, alo, chi = tp + tn, 1 - tn, 1 + tp
    theta, delta = 0.5 * (chi + alo), 0.5 * (chi - alo)
    cheb_ok = tn <= 0.5 and chi <= KAPPA_MAX * alo
    sk = np.sqrt(chi / max(alo, 0.25))
    sigma = (sk - 1) / (sk + 1)
    stop = EPS * EPS * nb * alo * alo
    on_cheb = not tau <= tau_neumann
    go = (cheb and cheb_ok) if on_cheb else True
    out = {"tau": tau, "tau_minus": tn, "chi": chi, "alo": alo, "cheb_ok": cheb_ok, "switch_ratios": [], "x": None}

    def apply(y):
        return Vu.T @ (w * (Vu @ y))

    napp, converged, switched = 0, False, False
    x, r = b.copy(), b.copy()
    if go and not on_cheb:
        sign, nprev = -1.0, nb
        while napp < KMAX:
            z = apply(r)
            napp += 1
            nr = float(z @ z)
            if nr * tau * tau <= stop:
                x = x + sign * z
                converged = True
                break
            if cheb_ok:
                out["switch_ratios"].append(nr / (max(sigma * sigma, 0.01) * nprev))
                if out["switch_ratios"][-1] > 1:
                    if not cheb:
                        break
                    r = sign * z
                    on_cheb = switched = True
                    break
            x = x + sign * z
            r = z
            sign, nprev = -sign, nr
    elif go:
        x = np.zeros_like(b)
    if cheb and go and on_cheb and not converged and cheb_ok:
        d = r / theta
        rho0 = phi = delta / theta
        while napp < KMAX:
            x = x + d
            z = apply(d)
            napp += 1
            r = r - d - z
            nr = float(r @ r)
            if nr * phi * phi <= stop:
                x = x + r / theta
                converged = True
                break
            irho = 1 / (2 * theta - rho0 * delta)
            rho1 = delta * irho
            d = 2 * irho * r + rho1 * rho0 * d
            rho0 = rho1
    if converged:
        out["path"] = "switch" if switched else "chebyshev" if on_cheb else "neumann"
        out["x"] = x
    else:
        out["path"] = "bounced" if cheb else "handed_on"
    out["applications"] = napp
    return out


def policy(Vu, w, cheb=True):
    """(path, applications of E): path is neumann, switch, chebyshev, handed_on (cheb=False only) or bounced."""
    d = policy_detail(Vu, w, cheb)
    return d["path"], d["applications"]


# -------------------------------------------------------------------------------------------------------------------- cases
# family: (block, tau_plus, tau_minus) -- the targets of sum |w| |v|^2 over the positive and the negative weights
FAMILIES = {
    "A": ("spread", 0.05, 0.0), "B": ("spread", 0.6, 0.0), "C": ("aligned", 0.7, 0.0),
    "D": ("spread", 1.5, 0.0), "Da": ("aligned", 2.5, 0.0), "E": ("spread", 6.0, 0.0),
    "F": ("spread", 0.15, 0.15), "G": ("spread", 0.4, 1.2), "H": ("aligned", 0.07 * 0.75, 0.93 * 0.75),
}


class Case:
    """The arrays of one solve, exactly as uploaded (float32 / int32 / int64), and what each row is."""

    def __init__(self, f, bias, rolled, V, side, bias_fixed, indptr, indices, values, family, labels):
        self.f, self.bias, self.rolled = f, int(bias), bool(rolled)
        self.ld, self.ldv, self.split = ld_for(f), ldv_of(f, bias), is_split(f, bias)
        self.V, self.side, self.bias_fixed = V, side, bias_fixed
        self.indptr, self.indices, self.values = indptr, indices, values
        self.family, self.labels = family, labels                   # per row: family name ("" for an empty row); {label: row}
        self.degree = np.diff(indptr)
        self.dmax = iter_dmax(f, bias)
        self.candidate = (self.degree >= 33) & (self.degree <= self.dmax)
        for a in (V, side, bias_fixed, indptr, indices, values):
            if a is not None:
                a.setflags(write=False)

    @property
    def n(self):
        return len(self.degree)

    def rows(self):
        return _row_inputs(self.V, self.side, self.bias_fixed, self.indptr, self.indices, self.values, self.f, self.rolled)

    def ref(self):
        return solve_rows_ref(self.V, self.side, self.bias_fixed, self.indptr, self.indices, self.values, self.f, self.rolled)

    def f32(self):
        return solve_rows_f32(self.V, self.side, self.bias_fixed, self.indptr, self.indices, self.values, self.f, self.rolled)

    def predict(self):
        """Per row policy_detail of the kernel that decides the row's fate (None for a row that is no candidate), and at
        ldv = 128 the two-wave stage's path as well."""
        final, stage1 = [None] * self.n, [None] * self.n
        for u, Vu, w in self.rows():
            if self.candidate[u]:
                final[u] = policy_detail(Vu, w, cheb=True)
                if self.ldv == 128:
                    stage1[u] = policy_detail(Vu, w, cheb=False)["path"]
        return final, stage1

    def expected_stats(self, final=None):
        """(done, bounced, applications, cheb) as wmf_plan_iter_stats reports them after one solve."""
        final = self.predict()[0] if final is None else final
        got = [p for p in final if p is not None]
        done = [p for p in got if p["path"] in SOLVED]
        return (len(done), len(got) - len(done), sum(p["applications"] for p in done),
                sum(1 for p in done if p["path"] != "neumann"))


def _fixed_side(f, bias, rolled, rng):
    """U float32 [600, f]: rows 0 .. 299 spread (Gaussian directions), 300 .. 599 aligned (one direction, 5 % of noise), norms
    0.03 (1 +- 0.1); rolled: the border feature is one number.  bias float32 [600], multiples of 2^-6, or None."""
    spread = rng.standard_normal((BLOCK, f))
    main = rng.standard_normal(f)
    main /= np.linalg.norm(main)
    noise = rng.standard_normal((BLOCK, f))
    aligned = main + 0.05 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    U = np.concatenate([spread, aligned])
    norms = ROW_NORM * (1 + 0.1 * (2 * rng.random(M_FIXED) - 1))
    if rolled:
        border = ROW_NORM / np.sqrt(f)
        body = U[:, :f - 1]
        body *= (np.sqrt(norms ** 2 - border ** 2) / np.linalg.norm(body, axis=1))[:, None]
        U = np.concatenate([body, np.full((M_FIXED, 1), border)], axis=1)
    else:
        U *= (norms / np.linalg.norm(U, axis=1))[:, None]
    b = (rng.integers(-16, 17, M_FIXED) / 64.0).astype(np.float32) if bias else None
    return U.astype(np.float32), b


def _layout(f, bias, rolled, U, b):
    """(V, side, bias_fixed) of the layout the library gathers at (f, bias)."""
    ld = ld_for(f)
    if not is_split(f, bias):
        V = np.zeros((M_FIXED, ld), dtype=np.float32)
        V[:, :f] = U
        return V, None, b
    V = np.ascontiguousarray(U[:, :f - 1])
    if rolled:
        assert f == 129
        word = b.view(np.uint32)
        raw = V.view(np.uint32)
        for j in range(16):
            raw[:, 8 * j] = (raw[:, 8 * j] & ~np.uint32(1)) | ((word >> np.uint32(2 * j)) & np.uint32(1))
            raw[:, 8 * j + 1] = (raw[:, 8 * j + 1] & ~np.uint32(1)) | ((word >> np.uint32(2 * j + 1)) & np.uint32(1))
        assert np.array_equal(rolled_bias(V), b)
    side = np.ascontiguousarray(np.stack([U[:, f - 1], b], axis=1))
    return V, side, None


def _family_of(name, d):
    return "Da" if name == "D" and d % 2 else name


def _make_row(rng, U64n2, fam, d, force=None):
    """(columns, weights) of one row: d distinct columns of the family's block; base weights 10 log(1 + c), c = 1 .. 7, scaled so
    that the positive / negative weights' sum |w| |v|^2 hit the family's targets, rounded to multiples of 2^-10."""
    block, tp, tn = FAMILIES[fam]
    off = 0 if block == "spread" else BLOCK
    cols = rng.choice(BLOCK, d, replace=False) + off
    if force is not None and force not in cols:
        cols[0] = force
    base = 10 * np.log(1 + rng.integers(1, 8, d))
    neg = np.zeros(d, dtype=bool)
    if tn > 0:
        share = tn / (tp + tn)
        k = min(max(int(round(share * d)), 1), d - 1)
        neg[rng.choice(d, k, replace=False)] = True
    n2 = U64n2[cols]
    w = np.where(neg, -base * tn / max((base * n2)[neg].sum(), 1e-300), base * tp / (base * n2)[~neg].sum())
    return cols.astype(np.int32), np.round(w * 1024) / 1024


def _assemble(f, bias, rolled, seed, plan):
    """plan: [(family, d)]; ('', 0) is an empty row.  The first spread row takes column 0, the first aligned one column m - 1."""
    rng = np.random.default_rng(seed)
    U, b = _fixed_side(f, bias, rolled, rng)
    V, side, bias_fixed = _layout(f, bias, rolled, U, b)
    U = features(V, side, f, rolled)[0]                              # (the rolled layout moved body values by an ulp)
    n2 = (U.astype(np.float64) ** 2).sum(axis=1)
    labels, cols_all, w_all, fams = {}, [], [], []
    blocks = {FAMILIES[fam.split(":")[0]][0] for fam, d in plan if d}
    forced = {k: v for k, v in (("spread", 0), ("aligned", M_FIXED - 1)) if k in blocks}
    wanted = set(forced.values())
    for u, (fam, d) in enumerate(plan):
        if d == 0:
            cols_all.append(np.zeros(0, dtype=np.int32))
            w_all.append(np.zeros(0))
            fams.append("")
            continue
        key = fam.split(":")[0]
        cols, w = _make_row(rng, n2, key, d, forced.pop(FAMILIES[key][0], None))
        if fam.endswith(":zero"):                                    # a stored zero (with a bias: w = -bias, p = 1 - bias)
            labels["stored_zero"] = u
            w[d // 2] = np.nan
        if fam.endswith(":dup"):                                     # a column stored twice: two separate entries
            labels["duplicate"] = u
            cols[d // 3] = cols[d // 3 + 5]
        cols_all.append(cols)
        w_all.append(w)
        fams.append(key)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols_all])]).astype(np.int64)
    indices = np.concatenate(cols_all).astype(np.int32)
    w = np.concatenate(w_all)
    bb = b.astype(np.float64)[indices] if bias else np.zeros(len(w))
    values = np.where(np.isnan(w), 0.0, w + bb)
    w = np.where(np.isnan(w), -bb, w)
    v32 = values.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), values)           # the stored value and ...
    assert np.array_equal((v32 - bb.astype(np.float32)).astype(np.float64), w)   # ... w = value - bias are exact in float32
    assert not forced and wanted <= set(indices.tolist())
    return Case(f, bias, rolled, V, side, bias_fixed, indptr, indices, v32, np.array(fams, dtype=object), labels)


# one width per shipped instantiation: (f, bias, rolled)
MAIN = ((81, 1, False), (100, 0, False), (101, 1, False), (125, 0, False), (128, 0, False), (129, 1, False), (129, 1, True),
        (161, 1, False), (192, 0, False), (200, 0, False), (256, 0, False), (260, 0, False))


def case_id(f, bias, rolled):
    return f"f{f}-b{int(bias)}" + ("-rolled" if rolled else "")


def _shuffled(plan, seed, empties=3):
    rng = np.random.default_rng(seed)
    plan = [plan[i] for i in rng.permutation(len(plan))]
    step = max(len(plan) // (empties + 1), 1)
    for k in range(empties):
        plan.insert((k + 1) * step + k, ("", 0))
    return plan


@functools.lru_cache(maxsize=None)
def build_case(f, bias, rolled=False):
    """A main case: families A and D at every d = 31 .. dmax + 2, the others at EDGES within [33, dmax], a row with a stored
    zero, one with a duplicated column, empty rows in between."""
    dmax = iter_dmax(f, bias)
    assert dmax
    plan = [(_family_of(fam, d), d) for fam in "AD" for d in range(31, dmax + 3)]
    plan += [(fam, d) for fam in "BCEFGH" for d in EDGES if 33 <= d <= dmax]
    plan += [("A:zero", 40), ("B:dup", 50)]
    return _assemble(f, bias, rolled, 9000 + 4 * f + 2 * int(bias) + int(rolled), _shuffled(plan, f))


@functools.lru_cache(maxsize=None)
def minor_case(f, bias):
    """The other widths of WIDTHS: A, C and D at the edge degrees (and dmax + 1), the two special rows, an empty row.  Where the
    width has no iteration kernel the edges up to 65 go to the elimination kernels."""
    dmax = iter_dmax(f, bias)
    top = dmax if dmax else 65
    plan = [(_family_of(fam, d), d) for fam in "ACD" for d in sorted({d for d in EDGES if d <= top} | {top + 1})]
    plan += [("A:zero", 40), ("C:dup", 50)]
    return _assemble(f, bias, False, 7000 + 2 * f + int(bias), _shuffled(plan, f, empties=1))


def minor_cases():
    main = {(f, b) for f, b, _ in MAIN}
    return [(f, b) for f in WIDTHS for b in (0, 1) if (f, b) not in main and f >= 2]


@functools.lru_cache(maxsize=None)
def pipeline_case(f, bias, rolled=False):
    """(distinct, clones, which): 32 distinct rows -- degrees alternating between 33, dmax and the slot edges, families A and D,
    at ldv = 128 all C so that the two-wave stage hands the whole list to the second stage's 512 workgroups -- and a list of
    4 cap + 37 clones of them, drawn at random so that a workgroup's consecutive rows differ."""
    dmax, eps = iter_dmax(f, bias), entries_per_slot(f, bias)
    slots = [d for s in range(1, dmax // eps + 1) for d in (eps * s, eps * s + 1) if 33 <= d <= dmax]
    rng = np.random.default_rng(50 + f)
    degs = [(33, dmax, int(rng.choice(slots)), int(rng.choice(slots)))[i % 4] for i in range(32)]
    fams = ["C"] * 32 if ldv_of(f, bias) == 128 else [_family_of("AD"[(i // 4 + i) % 2], i // 2) for i in range(32)]
    seed = 3000 + 4 * f + 2 * int(bias) + int(rolled)
    distinct = _assemble(f, bias, rolled, seed, list(zip(fams, degs)))
    n = 4 * grid_cap(f, bias) + 37
    which = rng.integers(0, 32, n)
    which[:32] = np.arange(32)
    deg = distinct.degree[which]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    take = np.concatenate([np.arange(distinct.indptr[k], distinct.indptr[k + 1]) for k in which])
    clones = Case(f, bias, rolled, distinct.V, distinct.side, distinct.bias_fixed, indptr, distinct.indices[take].copy(),
                  distinct.values[take].copy(), distinct.family[which], {})
    return distinct, clones, which


def single_row(case, u):
    """Row u of a case as a one-row case over the same fixed side."""
    lo, hi = case.indptr[u], case.indptr[u + 1]
    return Case(case.f, case.bias, case.rolled, case.V, case.side, case.bias_fixed, np.array([0, hi - lo], dtype=np.int64),
                case.indices[lo:hi].copy(), case.values[lo:hi].copy(), case.family[u:u + 1], {})


# --------------------------------------------------------------------------------------------------------------- the margins
def margins(case, final=None):
    """What keeps the float32 kernel on the path policy() predicts in float64, per candidate row; the CPU test asserts them.
    Returns [(row, what)] of the violations."""
    final = case.predict()[0] if final is None else final
    bad = []
    for u, Vu, w in case.rows():
        p = final[u]
        if p is None:
            continue
        tau, tn, chi, alo = p["tau"], p["tau_minus"], p["chi"], p["alo"]
        if 0.72 <= tau <= 0.88:
            # the Neumann limit decides nothing for a row that is bounced on either side of it: shown by running both
            lo_side = policy_detail(Vu, w, tau_neumann=0.72 * 0.999)["path"]
            hi_side = policy_detail(Vu, w, tau_neumann=0.88 * 1.001)["path"]
            if not (tn > 0.55 and lo_side == hi_side == p["path"] == "bounced"):
                bad.append((u, f"tau {tau:.4f}"))
        if 0.45 <= tn <= 0.55:
            bad.append((u, f"tau_minus {tn:.4f}"))
        if alo > 0 and 3.6 * alo <= chi <= 4.4 * alo:
            bad.append((u, f"chi / alpha {chi / alo:.4f}"))
        for k, ratio in enumerate(p["switch_ratios"]):
            if 1 / 1.5 < ratio < 1.5:
                bad.append((u, f"switch ratio {ratio:.3f} at application {k + 1}"))
        if p["path"] in SOLVED and p["applications"] > 17:
            bad.append((u, f"{p['applications']} applications"))
    return bad


def conditions(case):
    """cond_2(A_u) per row (1 for an empty row)."""
    out = np.ones(case.n)
    for u, Vu, w in case.rows():
        if len(w):
            Vu, w = Vu.astype(np.float64), w.astype(np.float64)
            ev = np.abs(np.linalg.eigvalsh(np.eye(case.f) + Vu.T @ (Vu * w[:, None])))
            out[u] = ev.max() / ev.min()
    return out
