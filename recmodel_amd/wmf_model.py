"""``WMF``: weighted matrix factorisation by alternating least squares, on MI355X.

Same class surface as RecModel/wmf_model.py:8-351 -- constructor, ``train`` / ``predict`` /
``rank``, ``recompute_factors[_bias][_par]``, public ``users`` / ``items`` host arrays -- with the
numerical work done by libwmf_hip.so through ``AlsEngine``.  ``cores`` selected a multiprocessing
pool in the reference; what its Pool variants change numerically is the dtype -- float64 rows stacked
without a cast -- and that is what ``cores > 1`` selects here too (the float64 device path,
``wmf_half_step_f64``).  There is no CPU fallback.
"""
import ctypes
import time

import numpy as np
import scipy.sparse
import torch

from . import _lib
from .base_model import RecModel, ranking_inputs
from .engine import AlsEngine, _ptr, _stream, audit_pass, audit_result


def _csr_parts(mat):
    mat = scipy.sparse.csr_matrix(mat) if not scipy.sparse.isspmatrix_csr(mat) else mat
    return (torch.from_numpy(mat.indptr.astype(np.int64)), torch.from_numpy(mat.indices.astype(np.int64)),
            torch.from_numpy(mat.data.astype(np.float32)))


# A float64 count matrix makes the reference solve every row system in float64 (NumPy's promotion at wmf_model.py:237-239).  The
# float32 row kernels reproduce that to the stated tolerance (5e-4 per row; measured 1e-5) while the confidence weights are of
# the benchmark's order; their error grows with the weights (cond(A_u) eps_f32: 1e-3 .. 6e-3 per row at weights of 1e6).  Above
# this weight a float64 count matrix therefore takes the float64 device path -- the reference's own arithmetic -- and the
# result is rounded to the model's dtype where the reference rounds it.
F64_ROW_WEIGHT = 1024.0

RECOMMEND_BATCH_USERS = 4096      # users per wmf_recommend_topn call of WMF.recommend (its workspace is 8 x 64 x topn bytes a user)
RECOMMEND_MAX_TOPN = 128          # WMF_RECOMMEND_MAX_TOPN of include/wmf_hip.h: beyond it recommend() takes the kernels of candidates()
CANDIDATES_MAX = 4096             # WMF_RECOMMEND_WIDE_MAX_TOPN of include/wmf_hip.h: the limit of candidates() and of recommend()'s device path
CANDIDATES_WS_BYTES = 1 << 30     # the workspace of one wmf_recommend_topn_wide call at most: candidates() takes fewer rows per call
SHELVES_MAX = 64                  # WMF_RECOMMEND_GROUPS_MAX of include/wmf_hip.h: the shelves of one recommend_shelves() call
MMR_MAX_POOL = 4096             # WMF_MMR_MAX_POOL of include/wmf_hip.h: the largest pool rerank_mmr() and recommend_diverse() take
ILS_MAX_WIDTH = 128               # WMF_ILS_MAX_WIDTH of include/wmf_hip.h: the longest list of intra_list_similarity()
RANKPOS_MAX_TARGETS = 16          # WMF_RANKPOS_MAX_TARGETS of include/wmf_hip.h: rank_positions() splits longer rows
EXPLAIN_MAX_TARGETS = 16          # WMF_EXPLAIN_MAX_TARGETS of include/wmf_hip.h: explain() splits longer target lists
POSTERIOR_MAX_DRAWS = 4096        # WMF_POSTERIOR_MAX_DRAWS of include/wmf_hip.h: the draws of a row in one posterior_draws() call
POSTERIOR_MAX_TARGETS = 4096      # WMF_POSTERIOR_MAX_TARGETS of include/wmf_hip.h: score_posterior() splits longer item lists


def _wrapped_ids(ids, n, what, dtype=np.int32):
    """The integer array ``ids`` as row numbers of a matrix of ``n`` rows -- a negative id counts from the end -- in ``dtype``;
    an IndexError that names ``what`` for an id outside [-n, n)."""
    if len(ids) and (ids.min() < -n or ids.max() >= n):
        raise IndexError(f"{what} index out of bounds")
    return np.where(ids < 0, ids + n, ids).astype(dtype)


def _target_ids(items, n_items, shaped):
    """``items`` as the int64 target array of a call on the row system: integer ids, ``shaped(array)`` the caller's own shape rule
    (it returns the 2-D array or raises), every id in [0, n_items) or -1 for an empty slot -- a ValueError otherwise."""
    tg = np.asarray(items)
    if tg.size and tg.dtype.kind not in "iu":
        raise ValueError(f"items must be integer ids, not {tg.dtype}")
    tg = shaped(tg).astype(np.int64)
    if tg.size and (tg.min() < -1 or tg.max() >= n_items):
        raise ValueError(f"items must be ids in [0, {n_items}) or -1 for an empty slot")
    return tg


def pack_allow_masks(masks):
    """bool [G, n] as the allow masks of include/wmf_hip.h: uint32 [G, ceil(n / 32)], item j is bit j & 31 of word j >> 5."""
    masks = np.atleast_2d(np.asarray(masks, dtype=bool))
    padded = np.zeros((masks.shape[0], 32 * max(1, (masks.shape[1] + 31) // 32)), dtype=bool)
    padded[:, :masks.shape[1]] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view('<u4').astype(np.uint32, copy=False)


class _Allow:
    """The ``allow`` / ``allow_idx`` arguments of the fused catalogue calls, checked on the host (every error a ValueError, before
    the GPU is asked for).  ``ids``: the list form (int32, sorted, unique; may be empty), or None; ``masks`` (bool [G, n]) and ``idx``
    (int32 per batch position, or None: mask 0 everywhere): the mask form.  ``as_mask``: an id list becomes its indicator mask."""

    def __init__(self, allow, allow_idx, n, n_batch, what, as_mask=False):
        self.n, self.ids, self.masks, self.idx = n, None, None, None
        if allow is None:
            raise ValueError("allow_idx needs a 2-D allow (one mask per row of it)")
        a = np.asarray(allow)
        if a.dtype == bool and a.ndim == 1:
            if allow_idx is not None:
                raise ValueError("allow_idx needs a 2-D allow (one mask per row of it); a 1-D mask is every row's")
            if len(a) != n:
                raise ValueError(f"a bool allow has one entry per {what} ({n}), not {len(a)}")
            self.masks = a[None, :]
        elif a.dtype == bool and a.ndim == 2:
            if a.shape[1] != n or a.shape[0] < 1:
                raise ValueError(f"a 2-D allow is [G >= 1, {n}] (one entry per {what}), not {a.shape}")
            if allow_idx is None:
                raise ValueError("a 2-D allow needs allow_idx: the mask of every batch position (-1: none)")
            idx = np.asarray(allow_idx)
            if idx.dtype == bool or not np.issubdtype(idx.dtype, np.integer) or idx.ndim != 1:
                raise ValueError("allow_idx must be a 1-D integer array")
            if len(idx) != n_batch:
                raise ValueError(f"allow_idx has one entry per batch position ({n_batch}), not {len(idx)}")
            if len(idx) and (idx.min() < -1 or idx.max() >= a.shape[0]):
                raise ValueError(f"allow_idx must lie in [-1, {a.shape[0]})")
            self.masks, self.idx = a, idx.astype(np.int32)
        elif a.ndim == 1 and (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            if allow_idx is not None:
                raise ValueError("allow_idx needs a 2-D allow (one mask per row of it), not a list of ids")
            a = a.astype(np.int64)
            if len(a) and (a.min() < -n or a.max() >= n):
                raise ValueError(f"allow holds an id outside [-{n}, {n})")
            self.ids = np.unique(np.where(a < 0, a + n, a)).astype(np.int32)
            if as_mask and len(self.ids):
                self.masks = np.zeros((1, n), dtype=bool)
                self.masks[0, self.ids] = True
                self.ids = None
        else:
            raise ValueError("allow must be a 1-D bool mask, a 1-D integer array of ids, or a 2-D bool array with allow_idx")

    @property
    def empty(self):
        return self.ids is not None and len(self.ids) == 0

    def allowed(self, b):
        """The eligible ids of batch position b, ascending."""
        if self.ids is not None:
            return self.ids
        g = 0 if self.idx is None else self.idx[b]
        return np.arange(self.n, dtype=np.int32) if g < 0 else np.flatnonzero(self.masks[g]).astype(np.int32)

    def upload(self):
        """The device arrays, made once per call.  Returns at(b0): the filter arguments of a C call whose batch starts at b0 --
        (allow_bits, allow_words, n_masks, allow_idx, cand_idx, n_cand)."""
        if self.ids is not None:
            cand = torch.from_numpy(self.ids).cuda()
            return lambda b0: (None, 0, 0, None, _ptr(cand), len(self.ids))
        bits = pack_allow_masks(self.masks)
        bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
        idx_d = None if self.idx is None else torch.from_numpy(self.idx).cuda()
        return lambda b0: (_ptr(bits_d), bits.shape[1], bits.shape[0], None if idx_d is None else _ptr(idx_d[b0:]), None, 0)

    @staticmethod
    def at(filt):
        """``filt.upload()``, or for None the filter arguments of a call without a filter."""
        return filt.upload() if filt is not None else (lambda b0: (None, 0, 0, None, None, 0))


class _Sample:
    """The sampling arguments of ``sample_items`` / ``sample_items_for``, checked on the host (every error a ValueError, before the
    GPU is asked for): ``n`` in 1..CANDIDATES_MAX, a finite ``temperature >= 0`` (> 0 with ``return_log_prob``), ``seed`` in [0, 2^64)
    and ``streams``, one uint64 per row (None: ``default``).  ``logz``: the rows' log-partitions, left here by _sample_scan."""

    def __init__(self, n, temperature, seed, streams, default, return_log_prob):
        self.n = int(n)
        if self.n < 1 or self.n > CANDIDATES_MAX:
            raise ValueError(f"n must be between 1 and {CANDIDATES_MAX}, not {self.n}")
        self.temperature = _checked_temperature(temperature, allow_zero=not return_log_prob)
        self.seed, self.streams = _checked_seed(seed), _checked_streams(streams, default)
        self.want_logp, self.logz = bool(return_log_prob), None

    def result(self, out_items, out_scores, good, one, return_scores):
        """What the sampling calls return: the items, then the scores with ``return_scores``, then with ``return_log_prob`` the
        float64 ``score / temperature - log Z`` of every pick (-inf in the padding); ``good``: the rows that have a list."""
        out = [out_items] + ([out_scores] if return_scores else [])
        if self.want_logp:
            logp = np.full(out_items.shape, -np.inf, dtype=np.float64)
            if self.logz is not None:
                with np.errstate(invalid="ignore"):                # (the padding: -inf - -inf)
                    got = out_scores.astype(np.float64) / np.float64(np.float32(self.temperature)) - self.logz.astype(np.float64)[:, None]
                keep = (out_items >= 0) & good[:, None]
                logp[keep] = got[keep]
            out.append(logp)
        out = [a[0] for a in out] if one else out
        return out[0] if len(out) == 1 else tuple(out)


class _Draw:
    """The noise arguments of ``posterior_draws`` / ``recommend_thompson_for``, checked on the host (every error a ValueError, before
    the GPU is asked for): ``draws`` in 1..POSTERIOR_MAX_DRAWS, a finite ``sigma >= 0``, ``seed`` in [0, 2^64) and ``streams``, one
    uint64 per row (None: ``default``)."""

    def __init__(self, draws, sigma, seed, streams, default):
        self.draws = int(draws)
        if self.draws < 1 or self.draws > POSTERIOR_MAX_DRAWS:
            raise ValueError(f"draws must be between 1 and {POSTERIOR_MAX_DRAWS}, not {self.draws}")
        s = float(sigma)
        if not 0 <= s <= float(np.finfo(np.float32).max):          # (a NaN fails the first)
            raise ValueError(f"sigma must be finite and >= 0, not {sigma!r}")
        self.sigma = float(np.float32(s))
        self.seed, self.streams = _checked_seed(seed), _checked_streams(streams, default)


def _checked_seed(seed):
    if isinstance(seed, (bool, float)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), not {seed!r}")
    return int(seed)


def _checked_streams(streams, default):
    """``streams`` as contiguous uint64, one per row (None: ``default``): a ValueError for anything but a 1-D array of integers in
    [0, 2^64) of ``len(default)``."""
    if streams is None:
        streams = default
    else:
        given, streams = streams, np.asarray(streams)
        if streams.dtype.kind not in "iu":                         # Python integers beyond int64 arrive as objects or floats
            streams = np.asarray(given, dtype=object)
            if streams.ndim == 1 and all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) and 0 <= x < 2 ** 64
                                         for x in streams):
                streams = np.array([int(x) for x in streams], dtype=np.uint64)
        if streams.dtype.kind not in "iu" or streams.ndim != 1 or len(streams) != len(default):
            raise ValueError(f"streams must be a 1-D integer array with one entry per row ({len(default)})")
        if len(streams) and streams.dtype != np.uint64 and streams.min() < 0:
            raise ValueError("streams must lie in [0, 2^64)")
    return np.ascontiguousarray(streams, dtype=np.uint64)


def _checked_temperature(temperature, allow_zero):
    t = float(temperature)
    if not 0 <= t <= float(np.finfo(np.float32).max) or (not allow_zero and np.float32(t) <= 0):    # (a NaN fails the first)
        raise ValueError(f"temperature must be finite and {'>= 0' if allow_zero else '> 0'}, not {temperature!r}")
    return t


def _padded(*shape):
    """The outputs every top-n call fills: int64 items padded with -1 and float32 scores padded with -inf, of ``shape``."""
    return np.full(shape, -1, dtype=np.int64), np.full(shape, -np.inf, dtype=np.float32)


def _topn_result(out_items, out_scores, one, return_scores):
    """... and what it returns: the items, with ``return_scores`` (items, scores); ``one``: the argument was an int, the leading
    axis goes."""
    if one:
        out_items, out_scores = out_items[0], out_scores[0]
    return (out_items, out_scores) if return_scores else out_items


def _topn_call(entry, head, n_cat, mid, topn, items_d, scores_d, count_d=None, moving=True):
    """``call`` of WMF._scan_batches for a top-n entry point of the library: entry(*head, ids, nb, n_cat, the first CSR's window if
    there is one, *mid(b0), topn, n_slices = 0, out_items, out_scores, out_count, workspace, its bytes, stream).  ``mid(b0)``: what
    the entry point takes between the seen lists and topn for a batch from b0 on -- the filter's tuple and the call's own.  The
    outputs are written from row b0 on; ``moving`` False: from row 0 (buffers of one window)."""
    def call(b0, nb, ids, csrs, *ws):
        o = b0 if moving else 0
        return entry(*head, ids, nb, n_cat, *(csrs[0] if csrs else ()), *mid(b0), topn, 0, _ptr(items_d[o:]),
                     _ptr(scores_d[o:]) if scores_d is not None else None, _ptr(count_d), *ws)
    return call


def _transformed_dtype(count_dtype, alpha, beta, pre_process_count):
    """dtype of the confidence weights the reference ends up with (wmf_model.py:119-123), by NumPy's own rules."""
    probe = np.ones(1, dtype=count_dtype)
    with np.errstate(all="ignore"):
        return (alpha * np.log(1 + beta * probe)).dtype if pre_process_count == 'log' else (alpha * probe).dtype


def audit_f64(K, X, Y, bias, gamma, indptr, indices, values, rows=False):
    """AlsEngine.audit for dense float64 device factors X [n, f] (the updated side), Y [m, f] and float64 CSR values: the two
    Gramians by float64 matmul, the pass over the CSR by wmf_half_step_audit_f64."""
    f = X.shape[1]
    Yt = Y
    if bias:
        Yt = Y.clone()
        Yt[:, 0] = 1.0
    G_fixed, G_side = Yt.T @ Yt, X.T @ X
    kernel = lambda xc, *rest: K.half_step_audit_f64(xc, Y, f, *rest)  # noqa: E731
    sums, eta = audit_pass(kernel, K, X, Y, f, bias, gamma, G_fixed, indptr, indices, values, X.shape[0], rows)
    out = audit_result((G_fixed * G_side).sum().cpu(), sums.cpu(), (gamma * G_side.diagonal().sum()).cpu())
    if rows:
        out["eta"] = eta
    return out


class _Float64Steps:
    """The two half steps of an iteration in float64 on the device (wmf_half_step_f64: RecModel/wmf_model.py:242-309) for
    `train(cores > 1)` on a float64 count matrix.  Factors live here as dense float64 device tensors; after every iteration
    float32 copies go to the engine, whose evaluation kernels compute the MSE train() stops on."""

    def __init__(self, model, eng, count_mat, alpha, beta, pre_process_count, store_float32=False):
        # store_float32: the reference's cores = 1 variants solve a float64 count matrix's rows in float64 and STORE float32
        # (wmf_model.py:217, :237-239) -- every half step's result is rounded to float32 before the next one reads it
        self.store_float32 = bool(store_float32)
        self.eng, self.K, self.bias, self.gamma = eng, eng.K, bool(model.bias), float(model.gamma)
        dev = eng.device
        C = scipy.sparse.csr_matrix(count_mat)
        self.csr = {}
        for side, mat in (("users", C), ("items", C.T.tocsr())):       # the transpose as the reference takes it (:128)
            vals = torch.from_numpy(np.ascontiguousarray(mat.data, dtype=np.float64)).to(dev)
            self.K.confidence_transform(vals, alpha, beta, 0 if pre_process_count == 'log' else 1)
            self.csr[side] = (torch.from_numpy(mat.indptr.astype(np.int64)).to(dev),
                              torch.from_numpy(mat.indices.astype(np.int32)).to(dev), vals, mat.shape[0])
        self.f = model.items.shape[1]
        self.X = {"items": torch.from_numpy(np.ascontiguousarray(model.items, dtype=np.float64)).to(dev), "users": None}
        n_max = max(C.shape)
        self.ws = torch.empty(self.K.half_step_f64_workspace_bytes(self.f, n_max, n_max), dtype=torch.uint8, device=dev)
        self.fail = torch.zeros(4, dtype=torch.int32, device=dev)

    def _half(self, side, fixed):
        indptr, indices, vals, n = self.csr[side]
        Y = self.X[fixed]
        out = torch.empty(n, self.f, dtype=torch.float64, device=Y.device)
        self.K.half_step_f64(Y, Y.shape[0], self.f, self.bias, indptr, indices, vals, n, self.gamma, out, self.ws, self.fail)
        self.X[side] = out.to(torch.float32).to(torch.float64) if self.store_float32 else out

    def audit(self, side, rows=False):
        """AlsEngine.audit on this object's float64 tensors (wmf_half_step_audit_f64)."""
        fixed = "items" if side == "users" else "users"
        indptr, indices, vals, n = self.csr[side]
        return audit_f64(self.K, self.X[side], self.X[fixed], self.bias, self.gamma, indptr, indices, vals, rows)

    def iteration(self, track=None):
        """track: a dict that receives the objective of each half step right after it (train(track_objective=True))."""
        self._half("users", "items")
        if track is not None:
            track["users"] = self.audit("users")
        self._half("items", "users")
        if track is not None:
            track["items"] = self.audit("items")
        fail = int(self.fail[0])
        if fail:
            self.fail.zero_()
            raise _lib.WmfNumericError(f"{fail} row systems were singular")
        for side in ("users", "items"):
            self.eng.set_factors(side, self.X[side].to(torch.float32))

    def factors(self):
        users, items = self.X["users"].cpu().numpy(), self.X["items"].cpu().numpy()
        return (users.astype(np.float32), items.astype(np.float32)) if self.store_float32 else (users, items)


class WMF(RecModel):

    def __init__(self, num_items, num_users, dim, gamma, weighted=None, bias=False, seed=1993, dtype='float32'):
        # wmf_model.py:10-23 -- the reference seeds the global legacy RNG and draws float64 uniforms
        np.random.seed(seed)
        self.bias = bias
        self.gamma = gamma
        if self.bias is False:
            self.items = np.random.random((num_items, dim)).astype(dtype=dtype)
        elif self.bias is True:
            self.items = np.random.random((num_items, (dim + 1))).astype(dtype=dtype)
        self.users = None
        self.num_users = num_users
        self.num_items = num_items
        self.dim = dim
        self.weighted = weighted
        self.dtype = dtype
        self._engine = None
        self._dev = None           # (key, users_t, items_t, f, ld): device copies of the public arrays for predict() / rank()
        self._inv_norms = {}       # {"users" / "items": float32 [rows] on the device}: inverse feature norms of the copies in _dev
        self._white = {}           # {gamma: W_white [f, ld] on the device}: whitening of the item copy in _dev (explain)
        self._groups = {}          # {id(array): (array, int32 [items] on the device)}: shelf assignments, kept as long as _dev is

    # ------------------------------------------------------------------ engine plumbing
    def _new_engine(self):
        return AlsEngine(self.num_users, self.num_items, self.dim, self.bias is True, self.gamma)

    def _device_factors(self):
        """Device copies of the public host arrays.  The arrays ``train`` leaves behind are read-only (assign a new array
        to change the factors): their copies are cached by identity.  A writable array -- the constructor's ``items``, or
        anything the caller assigned -- may have been edited in place since the last call, which the reference would see
        (it reads the arrays live, wmf_model.py:205-211), so such an array is uploaded again on every call."""
        _lib.require_gpu()
        frozen = not (self.users.flags.writeable or self.items.flags.writeable)
        key = (id(self.users), id(self.items), self.users.shape, self.items.shape)
        if self._dev is None or self._dev[0] != key or not frozen:
            lib = _lib.load()
            f = self.items.shape[1]
            ld = int(lib.wmf_ld_for(f))

            def up(a):
                t = torch.zeros(a.shape[0], ld, dtype=torch.float32, device="cuda")
                t[:, :f] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                return t
            self._dev = (key, up(self.users), up(self.items), f, ld)
            self._inv_norms = {}
            self._white = {}
            self._groups = {}
        return self._dev[1:]

    def _device_inv_norms(self, side):
        """(users_t, items_t, f, ld, inverse feature norms of ``side``): wmf_row_inv_norms on the device copy, kept exactly as
        long as that copy is -- by identity for the frozen arrays ``train`` leaves behind, computed again on every call for a
        writable array, which is uploaded again on every call."""
        users_t, items_t, f, ld = dev = self._device_factors()
        if side not in self._inv_norms:
            mat = users_t if side == "users" else items_t
            out = torch.empty(mat.shape[0], dtype=torch.float32, device="cuda")
            _lib.check(_lib.load().wmf_row_inv_norms(_ptr(mat), mat.shape[0], f, ld, int(self.bias is True), _ptr(out), _stream()))
            self._inv_norms[side] = out
        return dev + (self._inv_norms[side],)

    # ------------------------------------------------------------------ a7: predict
    def predict(self, users, items):
        """Scores for (user, item) pairs; one user or one item broadcasts.  wmf_model.py:191-211."""
        if (type(users) == list or type(users) == np.ndarray) and (type(items) == list or type(items) == np.ndarray):
            if len(users) != len(items):
                if not (len(users) == 1 or len(items) == 0):
                    raise ValueError("users and items need to have the same length or only one user / item needs to be provided.")
        u = np.atleast_1d(np.asarray(users)).astype(np.int32)
        i = np.atleast_1d(np.asarray(items)).astype(np.int32)
        if len(u) == 0 or len(i) == 0:
            return np.zeros(0, dtype=self.items.dtype)
        if len(u) != len(i) and len(i) == 1:
            i = np.repeat(i, len(u))
        u = _wrapped_ids(u, self.users.shape[0], "user or item")
        i = _wrapped_ids(i, self.items.shape[0], "user or item")
        users_t, items_t, f, ld = self._device_factors()
        lib = _lib.load()
        ut, it = torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()
        out = torch.empty(max(len(u), len(i)), dtype=torch.float32, device="cuda")
        _lib.check(lib.wmf_predict_pairs(_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True), _ptr(ut), len(u),
                                         _ptr(it), len(i), _ptr(out), _stream()))
        return out.cpu().numpy().astype(self.users.dtype, copy=False)

    # ------------------------------------------------------------------ a10: rank
    def rank(self, items, users, topn=None):
        """Top-n of the candidate ``items`` for a user, best first.  wmf_model.py:25-47.
        Scores and ordering both happen on the device (wmf_rank_topn); equal scores keep candidate order."""
        if topn is None:
            topn = len(items)
        if not type(items) == np.ndarray:
            items = np.array(items)
        n = len(items)
        keep = min(int(topn), n)
        if isinstance(users, list):
            # the reference recurses user by user (wmf_model.py:29-32); here all of them in one device call per batch
            if keep <= 0 or len(users) == 0:
                return [items[:0] for _ in users]
            return self._rank_many(items, users, keep)
        if keep <= 0:
            return items[:0]
        u = _wrapped_ids(np.array([int(np.asarray(users).reshape(-1)[0])]), self.users.shape[0], "user or item")
        idx = _wrapped_ids(np.asarray(items).astype(np.int64), self.items.shape[0], "user or item")
        users_t, items_t, f, ld = self._device_factors()
        lib = _lib.load()
        ut, it = torch.from_numpy(u).cuda(), torch.from_numpy(idx).cuda()
        ws_bytes = int(lib.wmf_rank_workspace_bytes(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        pos = torch.empty(keep, dtype=torch.int32, device="cuda")
        _lib.check(lib.wmf_rank_topn(_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True), _ptr(ut), _ptr(it), n, keep,
                                     _ptr(pos), None, _ptr(ws), ws_bytes, _stream()))
        return items[pos.cpu().numpy()]

    def _rank_many(self, items, users, keep):
        """rank() for a list of users: scores of 16 x 16 (user, candidate) tiles by MFMA, one segmented sort
        (wmf_rank_topn_batch), in batches of at most 2^26 scores."""
        n = len(items)
        u = _wrapped_ids(np.asarray(users).reshape(-1).astype(np.int64), self.users.shape[0], "user or item")
        idx = _wrapped_ids(np.asarray(items).astype(np.int64), self.items.shape[0], "user or item")
        users_t, items_t, f, ld = self._device_factors()
        lib = _lib.load()
        it = torch.from_numpy(idx).cuda()
        per = max(1, min(len(u), (1 << 26) // max(n, 1)))
        out = []
        ws = None
        for b0 in range(0, len(u), per):
            ub = torch.from_numpy(u[b0: b0 + per]).cuda()
            nu = ub.numel()
            need = int(lib.wmf_rank_batch_workspace_bytes(nu, n))
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            pos = torch.empty(nu * keep, dtype=torch.int32, device="cuda")
            _lib.check(lib.wmf_rank_topn_batch(_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True), _ptr(ub), nu, _ptr(it), n,
                                               keep, _ptr(pos), None, _ptr(ws), ws.numel(), _stream()))
            ph = pos.cpu().numpy().reshape(nu, keep)
            out.extend(items[ph[j]] for j in range(nu))
        return out

    # ------------------------------------------------------------------ a11: recommend
    def recommend(self, users, topn=10, exclude=None, return_scores=False, allow=None, allow_idx=None):
        """The ``topn`` best items of the whole catalogue for each of ``users`` (an int or a sequence of ints; negative
        indices count from the end, as in ``predict``), best first, equal scores in item order.  ``exclude``: a SciPy sparse
        matrix of shape [users of the model, items], e.g. the training matrix -- the stored entries of a user's row (stored
        zeros too) are never recommended to that user.  This is ``rank(np.delete(arange(n_items), seen_u), u, topn)`` for every
        user (RecModel/utils.py:3-17 on wmf_model.py:25-47) in one fused device pass per batch (wmf_recommend_topn).
        Returns int64 [len(users), topn], padded with -1 where a user has fewer eligible items; with ``return_scores`` also
        the float32 scores, padded with -inf.  An int user gives one row.
        ``allow`` restricts the catalogue (in stock, licensed, on a shelf); the form follows the argument, nothing is routed:
        a 1-D bool array of length items is one MASK for every row -- the whole catalogue is scored and the bit is tested where an
        item would enter a row's top-n (wmf_recommend_topn_filtered, mask form); a 1-D integer array of ids (any order,
        duplicates allowed, negative ids count from the end) is the LIST form, which reads and scores those rows only, at a cost
        proportional to ``len(ids)``; a 2-D bool array [G, items] with ``allow_idx`` -- one entry per entry of ``users``, values
        in [-1, G), -1: unrestricted -- gives every batch position its own mask, and a user may occur several times (the top 10
        of each of a user's five shelves is one call).  All three return, bit for bit, what ``exclude`` with the ineligible
        items added to every row returns.  An empty id list gives padding.  Which form: the mask form costs what the unfiltered
        call costs whatever the filter passes (2048 users, a million items, k = 128 + biases, topn 10 on an MI355X: 10.4 .. 11.4 ms
        against 11.0 ms, -4 .. +4.5 % on the scan kernel); the list form 0.55 ms for 99 ids, 1.03 ms for 10 000, 9.8 ms for
        500 000 and 18.2 ms for all million -- the two cross at about 575 000 ids, so a filter that passes more than half of the
        catalogue is faster as a mask (profiles/r19_recommend_filtered.json).
        ``topn`` beyond RECOMMEND_MAX_TOPN (128) and up to CANDIDATES_MAX (4096) is served on the device as well, by the kernels of
        ``candidates`` (wmf_recommend_topn_wide): the same scores and the same order.  Only beyond CANDIDATES_MAX are the users
        ranked one by one through ``rank`` and ``predict``."""
        return self._recommend(users, topn, exclude, return_scores, allow, allow_idx, False)

    def _recommend(self, users, topn, exclude, return_scores, allow, allow_idx, wide, mmr=None):
        """``recommend`` (wide False: the LDS kernels up to RECOMMEND_MAX_TOPN, the wide ones up to CANDIDATES_MAX, the host loop
        beyond) and ``candidates`` (wide True: the wide kernels for every topn).  ``mmr``: the checked (pool, lam, cosine) of
        ``recommend_diverse`` -- the pool of ``candidates`` re-ranked on the device (_diverse_scan); topn is then at most
        RECOMMEND_MAX_TOPN."""
        n_items = self.items.shape[0]
        one, u = self._checked_users(users, exclude)
        topn = int(topn)
        if topn < 1:
            raise ValueError(f"topn must be at least 1, not {topn}")
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_items, len(u), "item")
        _lib.require_gpu()
        out_items, out_scores = _padded(len(u), topn)
        seen = self._seen_rows(exclude, u)
        if len(u) == 0 or (filt is not None and filt.empty):
            pass
        elif topn > CANDIDATES_MAX:
            # beyond the device's buffers: the reference's formulation, user by user
            everything = np.arange(n_items, dtype=np.int32)
            for j, user in enumerate(u):
                cand = everything if filt is None else filt.allowed(j)
                if seen is not None:
                    cand = np.setdiff1d(cand, seen.indices[seen.indptr[j]:seen.indptr[j + 1]], assume_unique=False).astype(np.int32)
                best = self.rank(cand, int(user), topn) if len(cand) else cand
                out_items[j, :len(best)] = best
                if return_scores and len(best):
                    out_scores[j, :len(best)] = self.predict([int(user)], best)
        else:                                                      # (beyond RECOMMEND_MAX_TOPN: the wide kernels, as candidates())
            self._recommend_fused(u, topn, seen, out_items, out_scores if return_scores else None, filt, wide=wide or topn > RECOMMEND_MAX_TOPN,
                                  mmr=mmr)
        return _topn_result(out_items, out_scores, one, return_scores)

    def _checked_users(self, users, exclude):
        """The checks ``recommend`` and ``recommend_shelves`` make of ``users`` and ``exclude``, in their order: the ValueError of an
        ``exclude`` that is no sparse [users of the model, items], then the IndexError of a user outside the model.  Returns
        (``users`` was an int, the row of every batch position as int64)."""
        shape = (self.users.shape[0], self.items.shape[0])
        if exclude is not None and (not scipy.sparse.issparse(exclude) or exclude.shape != shape):
            raise ValueError(f"exclude must be a sparse matrix of shape {shape}, got {getattr(exclude, 'shape', None)}")
        return np.ndim(users) == 0, _wrapped_ids(np.atleast_1d(np.asarray(users)).reshape(-1).astype(np.int64), shape[0], "user", np.int64)

    @staticmethod
    def _seen_rows(exclude, u):
        """The rows ``u`` of a checked ``exclude``, a copy with sorted indices: the seen lists of the batch (None without either)."""
        if exclude is None or len(u) == 0:
            return None
        seen = scipy.sparse.csr_matrix(exclude)[u]
        seen.sort_indices()
        return seen

    def candidates(self, users, n=1000, exclude=None, return_scores=False, allow=None, allow_idx=None):
        """The candidate pool of a two-stage recommender, the lists behind Recall@500: the ``n`` best items of the whole catalogue
        for each of ``users``, 1 <= n <= CANDIDATES_MAX (4096; a ValueError otherwise, before the GPU is asked for).  The
        arguments, order, padding (-1 / -inf) and dtypes of ``recommend``; always served by wmf_recommend_topn_wide, whose running
        keys live in device memory instead of LDS, so for n <= RECOMMEND_MAX_TOPN it returns what ``recommend`` returns, bit for
        bit, from other kernels.  Rows per call are bounded by RECOMMEND_BATCH_USERS and by a workspace of CANDIDATES_WS_BYTES."""
        n = int(n)
        if n < 1 or n > CANDIDATES_MAX:
            raise ValueError(f"n must be between 1 and {CANDIDATES_MAX}, not {n}")
        return self._recommend(users, n, exclude, return_scores, allow, allow_idx, True)

    # ------------------------------------------------------------------ a18: sampled lists and their propensities
    def sample_items(self, users, n=10, temperature=1.0, seed=0, exclude=None, allow=None, allow_idx=None, streams=None,
                     return_scores=False, return_log_prob=False):
        """``n`` items for each of ``users`` DRAWN without replacement with probability proportional to ``exp(score / temperature)``
        over the items the user may see -- a Plackett-Luce draw, in draw order -- instead of the argmax of ``candidates``: an
        exploration slate, or hard negatives in proportion to the model's own softmax.  One scan of the catalogue per batch
        (wmf_sample_topn: the ``n`` largest of ``score + temperature * Gumbel noise``); ``users``, ``exclude``, ``allow`` /
        ``allow_idx``, padding and dtypes as in ``candidates``.  1 <= n <= CANDIDATES_MAX, ``temperature`` finite and >= 0, ``seed``
        an integer in [0, 2^64), ``streams`` one unsigned integer per entry of ``users``: a ValueError otherwise, before the GPU is
        asked for.  The noise of an item is a pure function of (``seed``, the row's stream, the item), and the default stream of a row
        is its USER ID: the same user under the same seed gets the same list however the batch is cut, and a user listed twice gets
        one list twice -- give ``streams`` to draw several lists for one user.  ``temperature == 0`` is ``candidates``.  Gumbel
        variates beyond [-2.81, 16.64] are never drawn: relative probabilities below about e^-16 are not resolved.
        Returns int64 [len(users), n], padded with -1; with ``return_scores`` also the MODEL's float32 scores of the picks (not the
        perturbed keys), padded with -inf; with ``return_log_prob`` also float64 ``score / temperature - log Z``, the log of the
        probability with which the item is drawn FIRST among the same eligible items (its single-draw propensity), -inf in the
        padding; ``log Z`` comes from wmf_log_partition in the same call, and ``temperature`` must then be > 0.  An int user gives
        one row."""
        n_items = self.items.shape[0]
        one, u = self._checked_users(users, exclude)
        sample = _Sample(n, temperature, seed, streams, u.astype(np.uint64), return_log_prob)
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_items, len(u), "item")
        _lib.require_gpu()
        out_items, out_scores = _padded(len(u), sample.n)
        if len(u) and not (filt is not None and filt.empty):
            users_t, items_t, f, ld = self._device_factors()
            out_items[:], scores = self._recommend_scan(users_t, items_t, f, ld, u, sample.n, self._seen_rows(exclude, u),
                                                        return_scores or sample.want_logp, filt, sample=sample)
            if scores is not None:
                out_scores[:] = scores
        return sample.result(out_items, out_scores, np.ones(len(u), dtype=bool), one, return_scores)

    def sample_items_for(self, count_rows, n=10, temperature=1.0, seed=0, exclude_history=True, allow=None, allow_idx=None, streams=None,
                         return_scores=False, return_log_prob=False, alpha=10, beta=1, pre_process_count='log'):
        """``sample_items`` for histories instead of user ids, as ``candidates_for`` is to ``candidates``: the rows of ``count_rows``
        are folded in on the device and ``n`` items are drawn for each.  The default stream of a row is its position in
        ``count_rows``.  A row whose fold-in failed is all -1 / -inf.  Bit for bit the output of ``sample_items`` on a model whose
        ``users`` are ``fold_in(count_rows)``, given the same streams."""
        mat, _ = self._foldin_arguments(count_rows, pre_process_count)
        sample = _Sample(n, temperature, seed, streams, np.arange(mat.shape[0], dtype=np.uint64), return_log_prob)
        return self._recommend_for(mat, sample.n, CANDIDATES_MAX, "n", exclude_history, return_scores, alpha, beta, pre_process_count,
                                   allow, allow_idx, sample=sample)

    def log_partition(self, users, temperature=1.0, exclude=None, allow=None, allow_idx=None):
        """``log sum_j exp(score(u, j) / temperature)`` over the items each of ``users`` may see (``exclude``, ``allow`` / ``allow_idx``
        as in ``recommend``): what turns a score into the log-probability of ``sample_items``.  One scan per batch
        (wmf_log_partition); ``temperature`` finite and > 0, a ValueError otherwise.  Returns float32 [len(users)], -inf for a user
        with nothing eligible; an int user gives a scalar."""
        n_items = self.items.shape[0]
        one, u = self._checked_users(users, exclude)
        T = float(np.float32(_checked_temperature(temperature, allow_zero=False)))
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_items, len(u), "item")
        _lib.require_gpu()
        out = np.full(len(u), -np.inf, dtype=np.float32)
        if len(u) and not (filt is not None and filt.empty):
            users_t, items_t, f, ld = self._device_factors()
            lib = _lib.load()
            seen = self._seen_rows(exclude, u)
            logz_d = torch.empty(len(u), dtype=torch.float32, device="cuda")
            head = (_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True))
            at = _Allow.at(filt)
            need = lambda rows: int(lib.wmf_log_partition_workspace_bytes(rows, 0))   # noqa: E731
            out[:] = self._scan_batches(
                u, [None if seen is None else (seen.indptr, seen.indices)], need, [logz_d],
                lambda b0, nb, ids, csrs, *ws: lib.wmf_log_partition(*head, ids, nb, n_items, *csrs[0], *at(b0), T, 0, _ptr(logz_d[b0:]), None, *ws),
                self._windows(len(u), need))[0]
        return out[0] if one else out

    # ------------------------------------------------------------------ a17: one list per shelf
    def recommend_shelves(self, users, groups, topn=10, exclude=None, return_scores=False, allow=None, allow_idx=None, n_groups=None):
        """The ``topn`` best items of EVERY SHELF for each of ``users``, from one scan of the catalogue (wmf_recommend_topn_grouped):
        ``groups`` is an integer array of length items, ``groups[j]`` the shelf (genre, department, carousel) of item j, a negative
        value: on no shelf, never returned.  G = ``n_groups``, or ``groups.max() + 1``; 1 <= G <= SHELVES_MAX (64), 1 <= topn <=
        RECOMMEND_MAX_TOPN (128), no id >= ``n_groups``, ``groups`` of an integer dtype and one entry per item: a ValueError
        otherwise, before the GPU is asked for.  Returns int64 [len(users), G, topn], best first within a shelf, padded with -1
        where a shelf has fewer eligible items; with ``return_scores`` also the float32 scores, padded with -inf.  An int user gives
        [G, topn].  ``users``, ``exclude`` and the order are those of ``recommend``; ``allow`` / ``allow_idx`` take its two mask
        forms, and an id list is turned into a mask on the host.  List (u, g) is, bit for bit, what ``recommend`` returns for u
        under the mask ``groups == g`` (and the row's allow mask): the route of ``recommend``'s docstring -- every user repeated
        once per shelf under a 2-D mask -- scores the catalogue G times, this call once.  Rows per call are bounded by
        RECOMMEND_BATCH_USERS and by CANDIDATES_WS_BYTES of the grouped workspace; the uploaded ``groups`` is kept beside the
        device copies of the factors while those are kept, when it is a read-only array (a writable one is uploaded per call).
        Which route (MI355X, a million items, k = 128 + biases, topn 10, 10 seen items per row; profiles/r22_recommend_shelves.json,
        DESIGN.md section 5): 2048 users x 16 shelves take 40.8 ms here and 160.8 ms as repeated rows under masks, 21.7 against
        40.1 ms at 4 shelves, 17.1 against 19.7 ms at 2, 151 ms at 64 (repeated rows: 91 ms for 256 of the users); over one plain
        scan (12.8 ms) that is 1.7 x at 4 shelves, 3.2 x at 16, 11.8 x at 64.  Use this call for batches from two shelves on; the
        repeated rows of ``recommend`` are faster for a single shelf (10.8 against 14.3 ms) and for a handful of users (16 users x
        16 shelves: 5.0 against 14.1 ms), whose repeated rows fill the device where one 16-row wave per slice does not."""
        n_items = self.items.shape[0]
        g32, G, topn = self._shelf_arguments(groups, n_groups, topn, n_items)
        one, u = self._checked_users(users, exclude)
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_items, len(u), "item", as_mask=True)
        _lib.require_gpu()
        out_items, out_scores = _padded(len(u), G, topn)
        if len(u) and not (filt is not None and filt.empty):
            users_t, items_t, f, ld = self._device_factors()
            out_items[:], scores = self._shelves_scan(users_t, items_t, f, ld, u, groups, g32, G, topn, self._seen_rows(exclude, u), return_scores, filt)
            if return_scores:
                out_scores[:] = scores
        return _topn_result(out_items, out_scores, one, return_scores)

    def recommend_capped(self, users, groups, topn=10, per_group=2, exclude=None, return_scores=False, allow=None, allow_idx=None):
        """The ``topn`` best items overall with at most ``per_group`` of any shelf -- the commonest business rule on top of
        ``recommend_shelves``, whose ``users``, ``groups`` (G = ``groups.max() + 1``), ``exclude`` and ``allow`` it takes.  Exact by
        construction: an item of the capped list is among its shelf's min(per_group, topn) best, so the list is the merge of
        ``recommend_shelves(..., topn=min(per_group, topn))`` -- a row's G x q keys sorted by (score descending, -0.0 equal to +0.0;
        item ascending) on the host, the first ``topn`` taken.  Items on no shelf (a negative group) are NOT eligible: give them a
        shelf of their own to keep them.  ``per_group >= topn`` with every item on one shelf is ``recommend``.  Returns int64
        [len(users), topn] padded with -1, with ``return_scores`` also the float32 scores padded with -inf; an int user gives one
        row."""
        topn, per_group = int(topn), int(per_group)
        if topn < 1 or topn > RECOMMEND_MAX_TOPN:
            raise ValueError(f"topn must be between 1 and {RECOMMEND_MAX_TOPN}, not {topn}")
        if per_group < 1:
            raise ValueError(f"per_group must be at least 1, not {per_group}")
        one = np.ndim(users) == 0
        items, scores = self.recommend_shelves(np.atleast_1d(np.asarray(users)).reshape(-1), groups, min(per_group, topn), exclude, True,
                                               allow, allow_idx)
        B = items.shape[0]
        items, scores = items.reshape(B, -1), scores.reshape(B, -1)
        last = np.where(items < 0, np.iinfo(np.int64).max, items)     # padding behind every item, whatever its score
        order = np.lexsort((last, -(scores + np.float32(0))), axis=-1)[:, :topn]
        out_items, out_scores = _padded(B, topn)
        out_items[:, :order.shape[1]] = np.take_along_axis(items, order, axis=1)
        out_scores[:, :order.shape[1]] = np.take_along_axis(scores, order, axis=1)
        return _topn_result(out_items, out_scores, one, return_scores)

    @staticmethod
    def _shelf_arguments(groups, n_groups, topn, n_items):
        """The checks the shelf calls share, before the GPU is asked for; returns (groups as int32 with every no-shelf value -1, G,
        topn)."""
        g = np.asarray(groups)
        if g.dtype == bool or not np.issubdtype(g.dtype, np.integer) or g.ndim != 1:
            raise ValueError("groups must be a 1-D integer array: the shelf of every item, negative for none")
        if len(g) != n_items:
            raise ValueError(f"groups has one entry per item ({n_items}), not {len(g)}")
        top = int(g.max()) if len(g) else -1
        G = int(n_groups) if n_groups is not None else top + 1
        if G < 1 or G > SHELVES_MAX:
            raise ValueError(f"the number of shelves must be between 1 and {SHELVES_MAX}, not {G}")
        if top >= G:
            raise ValueError(f"groups holds the id {top}, beyond n_groups = {G}")
        topn = int(topn)
        if topn < 1 or topn > RECOMMEND_MAX_TOPN:
            raise ValueError(f"topn must be between 1 and {RECOMMEND_MAX_TOPN}, not {topn}")
        return np.where(g < 0, -1, g).astype(np.int32), G, topn

    def _device_groups(self, groups, g32):
        """The device copy of a shelf assignment (after _device_factors): kept beside the factors' copies, under their rule -- by
        identity for a read-only array, while the factors' copies are kept; a writable array is uploaded on every call."""
        if isinstance(groups, np.ndarray) and not groups.flags.writeable and not (self.users.flags.writeable or self.items.flags.writeable):
            hit = self._groups.get(id(groups))
            if hit is None or hit[0] is not groups:
                hit = self._groups[id(groups)] = (groups, torch.from_numpy(g32).cuda())     # (the array is held: its id stays its own)
            return hit[1]
        return torch.from_numpy(g32).cuda()

    def _shelves_scan(self, users_t, items_t, f, ld, u, groups, g32, G, topn, seen, want_scores, filt):
        """wmf_recommend_topn_grouped on the rows ``u`` of the device matrix ``users_t`` in batches (_scan_batches), in windows
        whose workspace stays within CANDIDATES_WS_BYTES (one row at least).  Returns the host (items [B, G, topn], scores or
        None)."""
        lib = _lib.load()
        n_items = self.items.shape[0]
        items_d = torch.empty(len(u), G, topn, dtype=torch.int32, device="cuda")
        scores_d = torch.empty(len(u), G, topn, dtype=torch.float32, device="cuda") if want_scores else None
        head = (_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True))
        groups_d = self._device_groups(groups, g32)
        at = _Allow.at(filt)
        need = lambda rows: int(lib.wmf_recommend_grouped_workspace_bytes(rows, G, topn, 0))   # noqa: E731
        call = _topn_call(lib.wmf_recommend_topn_grouped, head, n_items, lambda b0: (*at(b0)[:4], _ptr(groups_d), G), topn, items_d, scores_d)
        return self._scan_batches(u, [None if seen is None else (seen.indptr, seen.indices)], need, [items_d, scores_d], call,
                                  self._windows(len(u), need))

    # ------------------------------------------------------------------ a15: diversified lists
    @staticmethod
    def _mmr_arguments(topn, pool, lam, metric):
        """The checks the diversified calls share, before the GPU is asked for; returns (topn, pool, lam, cosine)."""
        if metric not in ('cosine', 'dot'):
            raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
        topn = int(topn)
        if topn < 1 or topn > RECOMMEND_MAX_TOPN:
            raise ValueError(f"topn must be between 1 and {RECOMMEND_MAX_TOPN}, not {topn}")
        pool = min(10 * topn, MMR_MAX_POOL) if pool is None else int(pool)
        if pool < 1 or pool > MMR_MAX_POOL:
            raise ValueError(f"pool must be between 1 and {MMR_MAX_POOL}, not {pool}")
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:                                  # (a NaN fails both comparisons)
            raise ValueError(f"lam must lie in [0, 1], not {lam}")
        return topn, pool, lam, metric == 'cosine'

    def recommend_diverse(self, users, topn=10, pool=None, lam=0.7, metric='cosine', exclude=None, allow=None, allow_idx=None,
                          return_scores=False):
        """``recommend`` with the near-duplicates thinned out: the ``pool`` best items of each user (``candidates``, with its
        ``exclude`` / ``allow`` / ``allow_idx``) re-ranked by greedy Maximal Marginal Relevance -- items are picked one by one, each
        the remaining candidate with the largest ``lam * score - (1 - lam) * (highest similarity to the items picked so far)``,
        equal values in pool order.  ``metric``: the similarity, 'cosine' or 'dot' over the item features (the bias column is none).
        ``pool=None`` is ``min(10 * topn, MMR_MAX_POOL)``; 1 <= topn <= RECOMMEND_MAX_TOPN, topn <= pool <= MMR_MAX_POOL (4096) and
        0 <= lam <= 1, a ValueError otherwise, before the GPU is asked for.  ``lam == 1`` returns exactly what ``recommend`` returns;
        ``lam == 0`` keeps the best item and then spreads out.  The pool never leaves the device (wmf_recommend_topn_wide into
        wmf_rerank_mmr, per window of rows); one copy back.  Returns int64 [len(users), topn], padded with -1; with
        ``return_scores`` also the items' float32 scores (those of ``recommend``, not the marginal values), padded with -inf."""
        topn, pool, lam, cosine = self._mmr_arguments(topn, pool, lam, metric)
        if pool < topn:
            raise ValueError(f"pool ({pool}) must be at least topn ({topn})")
        return self._recommend(users, topn, exclude, return_scores, allow, allow_idx, True, mmr=(pool, lam, cosine))

    def rerank_mmr(self, pool_items, pool_scores, topn=10, lam=0.7, metric='cosine', pool_count=None, return_scores=False):
        """Greedy Maximal Marginal Relevance over candidate pools of the caller's: ``pool_items`` [B, pool] item ids and
        ``pool_scores`` [B, pool] their relevances, taken as given, e.g. the two outputs of ``candidates`` or the scores of another
        model.  NumPy arrays, or torch tensors on the device (int32 ids, float32 scores), which are used as they are.  The candidates
        of a row are its leading ``pool_count[b]`` entries; ``pool_count=None``: the entries before the row's first negative id (the
        -1 padding of ``candidates``).  An id listed twice is two candidates.  ``topn``, ``lam``, ``metric`` and the order as in
        ``recommend_diverse``; the pool may be shorter than ``topn`` (the rows are padded).  Returns int64 [B, topn], padded with
        -1; with ``return_scores`` also the float32 relevances of the picks, padded with -inf.  One-dimensional inputs are one row."""
        topn, _, lam, cosine = self._mmr_arguments(topn, 1, lam, metric)
        if self.users is None:                                      # (the device copies are of both matrices; as in similar_items)
            raise AttributeError("the model has no user factors yet: train it, or assign users, before re-ranking")
        n_items = self.items.shape[0]
        on_device = torch.is_tensor(pool_items)
        if on_device != torch.is_tensor(pool_scores) or (pool_count is not None and torch.is_tensor(pool_count) != on_device):
            raise ValueError("pool_items, pool_scores and pool_count must all be host arrays or all be device tensors")
        if not on_device:
            pool_items, pool_scores = np.asarray(pool_items), np.asarray(pool_scores)
            if pool_items.dtype == bool or not np.issubdtype(pool_items.dtype, np.integer):
                raise ValueError("pool_items must be an integer array")
        elif pool_items.dtype != torch.int32 or pool_scores.dtype != torch.float32 or not pool_items.is_cuda or not pool_scores.is_cuda:
            raise ValueError("device pools are int32 ids and float32 scores on the GPU")
        one = pool_items.ndim == 1
        if one:
            pool_items, pool_scores = pool_items[None, :], pool_scores[None, :] if pool_scores.ndim == 1 else pool_scores
        if pool_items.ndim != 2 or tuple(pool_items.shape) != tuple(pool_scores.shape):
            raise ValueError(f"pool_items and pool_scores must have one shape [B, pool], not {tuple(pool_items.shape)} and {tuple(pool_scores.shape)}")
        B, pool = int(pool_items.shape[0]), int(pool_items.shape[1])
        if pool < 1 or pool > MMR_MAX_POOL:
            raise ValueError(f"the pool must hold between 1 and {MMR_MAX_POOL} entries a row, not {pool}")
        if not on_device:
            if pool_items.size and (pool_items.min() < -1 or pool_items.max() >= n_items):
                raise IndexError("item index out of bounds")
            if np.isnan(np.asarray(pool_scores, dtype=np.float32)).any():
                raise ValueError("pool_scores holds a NaN")
        if pool_count is not None:
            if tuple(pool_count.shape) != (B,):
                raise ValueError(f"pool_count has one entry per row ({B}), not shape {tuple(pool_count.shape)}")
            if not on_device:
                pool_count = np.asarray(pool_count)
                if pool_count.dtype == bool or not np.issubdtype(pool_count.dtype, np.integer):
                    raise ValueError("pool_count must be an integer array")
                if B and (pool_count.min() < 0 or pool_count.max() > pool):
                    raise ValueError(f"pool_count must lie in [0, {pool}]")
            elif pool_count.dtype != torch.int32 or not pool_count.is_cuda:
                raise ValueError("a device pool_count is int32 on the GPU")
        _lib.require_gpu()
        out_items, out_scores = _padded(B, topn)
        if B:
            if cosine:
                _, items_t, f, ld, norms = self._device_inv_norms("items")
            else:
                (_, items_t, f, ld), norms = self._device_factors(), None
            if not on_device:
                pool_items = torch.from_numpy(np.ascontiguousarray(pool_items, dtype=np.int32)).cuda()
                pool_scores = torch.from_numpy(np.ascontiguousarray(pool_scores, dtype=np.float32)).cuda()
                pool_count = None if pool_count is None else torch.from_numpy(np.ascontiguousarray(pool_count, dtype=np.int32)).cuda()
            pool_items, pool_scores = pool_items.contiguous(), pool_scores.contiguous()
            if pool_count is None:                                 # the entries before the first negative id
                pool_count = (pool_items >= 0).to(torch.int32).cumprod(dim=1).sum(dim=1).to(torch.int32)
            items_d = torch.empty(B, topn, dtype=torch.int32, device="cuda")
            scores_d = torch.empty(B, topn, dtype=torch.float32, device="cuda") if return_scores else None
            _lib.check(_lib.load().wmf_rerank_mmr(_ptr(items_t), n_items, f, ld, int(self.bias is True), _ptr(norms), _ptr(pool_items),
                                                  _ptr(pool_scores), _ptr(pool_count.contiguous()), B, pool, lam, topn, _ptr(items_d),
                                                  _ptr(scores_d), None, None, _stream()))
            out_items[:] = items_d.cpu().numpy()
            if return_scores:
                out_scores[:] = scores_d.cpu().numpy()
        return _topn_result(out_items, out_scores, one, return_scores)

    def intra_list_similarity(self, item_lists, metric='cosine'):
        """How alike the items of each list are, the measure a diversified list is judged by: for every row of ``item_lists``
        ([B, width <= ILS_MAX_WIDTH] item ids, e.g. what ``recommend`` or ``recommend_diverse`` returned; a NumPy array, or an int32
        torch tensor on the device, used as it is) the mean and the largest similarity over the unordered pairs of its entries.
        The first negative entry ends a list (the -1 padding); an id listed twice is two entries.  ``metric``: 'cosine' or 'dot'
        over the item features.  Returns (mean, max), float32 [B]: 0 and -inf for a list of fewer than two items.  One workgroup
        per list on the device (wmf_intra_list_similarity).  A one-dimensional input is one list and gives two scalars."""
        if metric not in ('cosine', 'dot'):
            raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
        if self.users is None:                                      # (the device copies are of both matrices; as in similar_items)
            raise AttributeError("the model has no user factors yet: train it, or assign users, before asking for similarities")
        n_items = self.items.shape[0]
        on_device = torch.is_tensor(item_lists)
        if not on_device:
            item_lists = np.asarray(item_lists)
            if item_lists.dtype == bool or not np.issubdtype(item_lists.dtype, np.integer):
                raise ValueError("item_lists must be an integer array")
        elif item_lists.dtype != torch.int32 or not item_lists.is_cuda:
            raise ValueError("a device item_lists is int32 on the GPU")
        one = item_lists.ndim == 1
        if one:
            item_lists = item_lists[None, :]
        if item_lists.ndim != 2 or item_lists.shape[1] < 1 or item_lists.shape[1] > ILS_MAX_WIDTH:
            raise ValueError(f"item_lists must be [B, width] with 1 <= width <= {ILS_MAX_WIDTH}, not {tuple(item_lists.shape)}")
        if not on_device and item_lists.size and (item_lists.min() < -1 or item_lists.max() >= n_items):
            raise IndexError("item index out of bounds")
        _lib.require_gpu()
        B, width = int(item_lists.shape[0]), int(item_lists.shape[1])
        mean, top = np.zeros(B, dtype=np.float32), np.full(B, -np.inf, dtype=np.float32)
        if B:
            if metric == 'cosine':
                _, items_t, f, ld, norms = self._device_inv_norms("items")
            else:
                (_, items_t, f, ld), norms = self._device_factors(), None
            lists_d = item_lists.contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(item_lists, dtype=np.int32)).cuda()
            count_d = (lists_d >= 0).to(torch.int32).cumprod(dim=1).sum(dim=1).to(torch.int32)
            mean_d = torch.empty(B, dtype=torch.float32, device="cuda")
            top_d = torch.empty(B, dtype=torch.float32, device="cuda")
            _lib.check(_lib.load().wmf_intra_list_similarity(_ptr(items_t), n_items, f, ld, int(self.bias is True), _ptr(norms), _ptr(lists_d),
                                                             _ptr(count_d), B, width, _ptr(mean_d), _ptr(top_d), _stream()))
            mean, top = mean_d.cpu().numpy(), top_d.cpu().numpy()
        return (mean[0], top[0]) if one else (mean, top)

    def _scan_batches(self, ids, csrs, ws_bytes, outs, call, max_rows=None):
        """The batch loop of the fused catalogue calls (recommend, the neighbours, rank_positions): windows of
        RECOMMEND_BATCH_USERS rows, all enqueued on one stream, one copy to the host at the end.  ``ids``: the row of the factors
        each batch position reads; ``csrs``: per-position lists as (indptr, indices), or None, uploaded once; ``ws_bytes(rows)``:
        the workspace of a batch; ``outs``: the device outputs (None: not asked for).  ``call(b0, nb, ids, csrs, ws, ws_bytes,
        stream)`` enqueues the nb positions from b0 on: pointers to the ids from b0 on and, for each CSR, to the window of its
        pointers and to its one indices array (None, None without it) -- row b of the batch is row b0 + b.  ``max_rows``: a
        further bound on the rows of a window.  Returns the host copies of ``outs``."""
        n = len(ids)
        ids_d = torch.from_numpy(ids.astype(np.int32)).cuda()
        csrs_d = [None if c is None else (torch.from_numpy(c[0].astype(np.int64)).cuda(),         # (one spare index: never empty)
                                          torch.from_numpy(np.append(c[1], 0).astype(np.int32)).cuda()) for c in csrs]
        per = max(1, min(int(RECOMMEND_BATCH_USERS), int(max_rows or RECOMMEND_BATCH_USERS)))
        nbytes = int(ws_bytes(min(per, n)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for b0 in range(0, n, per):
            nb = min(per, n - b0)
            windows = [(_ptr(c[0][b0: b0 + nb + 1]), _ptr(c[1])) if c else (None, None) for c in csrs_d]
            _lib.check(call(b0, nb, _ptr(ids_d[b0:]), windows, _ptr(ws), nbytes, _stream()))
        return [o if o is None else o.cpu().numpy() for o in outs]

    def _recommend_fused(self, u, topn, seen, out_items, out_scores, filt=None, wide=False, mmr=None):
        """wmf_recommend_topn in batches (_scan_batches); the rows of ``seen`` are those of ``u``.  ``filt``: an _Allow, then
        wmf_recommend_topn_filtered.  ``wide``: wmf_recommend_topn_wide, with or without a filter.  ``mmr``: _diverse_scan."""
        users_t, items_t, f, ld = self._device_factors()
        out_items[:], scores = self._recommend_scan(users_t, items_t, f, ld, u, topn, seen, out_scores is not None, filt, wide, mmr)
        if out_scores is not None:
            out_scores[:] = scores

    @staticmethod
    def _windows(n, need):
        """The rows of a window of ``n`` positions whose workspace ``need(rows)`` stays within CANDIDATES_WS_BYTES (one row at
        least): the wide, diversified and shelf scans hand it to _scan_batches."""
        rows = max(1, min(n, int(RECOMMEND_BATCH_USERS)))
        while rows > 1 and need(rows) > CANDIDATES_WS_BYTES:       # (it grows with the rows: halve until a window fits)
            rows //= 2
        return rows

    def _diverse_scan(self, users_t, items_t, f, ld, u, topn, seen, want_scores, filt, mmr):
        """``candidates`` re-ranked without leaving the device: per window of _scan_batches, wmf_recommend_topn_wide(topn = pool)
        into pool buffers of one window's rows -- reused by the next window, which the stream orders behind this one -- and
        wmf_rerank_mmr from those buffers, the pool's out_count as its pool_count, into the outputs.  One copy back."""
        pool, lam, cosine = mmr
        lib = _lib.load()
        norms = self._device_inv_norms("items")[4] if cosine else None
        need = lambda rows: int(lib.wmf_recommend_wide_workspace_bytes(rows, pool, 0))   # noqa: E731
        rows = self._windows(len(u), need)
        pool_i = torch.empty(rows, pool, dtype=torch.int32, device="cuda")
        pool_s = torch.empty(rows, pool, dtype=torch.float32, device="cuda")
        pool_c = torch.empty(rows, dtype=torch.int32, device="cuda")
        items_d = torch.empty(len(u), topn, dtype=torch.int32, device="cuda")
        scores_d = torch.empty(len(u), topn, dtype=torch.float32, device="cuda") if want_scores else None
        n_items = self.items.shape[0]
        scan = _topn_call(lib.wmf_recommend_topn_wide, (_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True)), n_items, _Allow.at(filt),
                          pool, pool_i, pool_s, pool_c, moving=False)

        def call(b0, nb, ids, csrs, *ws):
            rc = scan(b0, nb, ids, csrs, *ws)
            if rc != _lib.WMF_OK:
                return rc
            return lib.wmf_rerank_mmr(_ptr(items_t), n_items, f, ld, int(self.bias is True), _ptr(norms), _ptr(pool_i), _ptr(pool_s), _ptr(pool_c),
                                      nb, pool, lam, topn, _ptr(items_d[b0:]), _ptr(scores_d[b0:]) if scores_d is not None else None, None,
                                      None, ws[-1])
        return self._scan_batches(u, [None if seen is None else (seen.indptr, seen.indices)], need, [items_d, scores_d], call, rows)

    def _sample_scan(self, users_t, items_t, f, ld, u, n, seen, want_scores, filt, sample):
        """wmf_sample_topn on the rows ``u`` of the device matrix ``users_t`` in batches (_scan_batches), the streams' window moving
        with the ids'; with ``sample.want_logp`` wmf_log_partition follows in the same window, on the same stream and workspace, and
        the rows' log Z is left in ``sample.logz``.  Returns the host (items, scores or None)."""
        lib = _lib.load()
        n_items = self.items.shape[0]
        items_d = torch.empty(len(u), n, dtype=torch.int32, device="cuda")
        scores_d = torch.empty(len(u), n, dtype=torch.float32, device="cuda") if want_scores else None
        logz_d = torch.empty(len(u), dtype=torch.float32, device="cuda") if sample.want_logp else None
        streams_d = torch.from_numpy(sample.streams.view(np.int64)).cuda()
        head = (_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True))
        at = _Allow.at(filt)
        T = float(np.float32(sample.temperature))

        def need(rows):
            most = int(lib.wmf_sample_workspace_bytes(rows, n, 0))
            return max(most, int(lib.wmf_log_partition_workspace_bytes(rows, 0))) if sample.want_logp else most

        def call(b0, nb, ids, csrs, *ws):
            rc = lib.wmf_sample_topn(*head, ids, nb, n_items, *csrs[0], *at(b0), n, 0, T, sample.seed, _ptr(streams_d[b0:]), _ptr(items_d[b0:]),
                                     _ptr(scores_d[b0:]) if want_scores else None, None, None, *ws)
            if rc != _lib.WMF_OK or logz_d is None:
                return rc
            return lib.wmf_log_partition(*head, ids, nb, n_items, *csrs[0], *at(b0), T, 0, _ptr(logz_d[b0:]), None, *ws)
        items, scores, sample.logz = self._scan_batches(u, [None if seen is None else (seen.indptr, seen.indices)], need,
                                                        [items_d, scores_d, logz_d], call, self._windows(len(u), need))
        return items, scores

    def _recommend_scan(self, users_t, items_t, f, ld, u, topn, seen, want_scores, filt, wide=False, mmr=None, sample=None):
        """The fused top-n of the rows ``u`` of the device matrix ``users_t`` in batches (_scan_batches): wmf_recommend_topn, or with
        a filter wmf_recommend_topn_filtered -- its masks or ids uploaded once, the allow_idx window moving with the ids'.  Returns
        the host (items, scores or None).  ``wide``: wmf_recommend_topn_wide for either, in windows whose workspace stays within
        CANDIDATES_WS_BYTES (one row at least).  ``mmr``: _diverse_scan instead; ``sample``: _sample_scan instead."""
        if sample is not None:
            return self._sample_scan(users_t, items_t, f, ld, u, topn, seen, want_scores, filt, sample)
        if mmr is not None:
            return self._diverse_scan(users_t, items_t, f, ld, u, topn, seen, want_scores, filt, mmr)
        lib = _lib.load()
        items_d = torch.empty(len(u), topn, dtype=torch.int32, device="cuda")
        scores_d = torch.empty(len(u), topn, dtype=torch.float32, device="cuda") if want_scores else None
        if wide:
            entry, mid, ws_bytes = lib.wmf_recommend_topn_wide, _Allow.at(filt), lib.wmf_recommend_wide_workspace_bytes
        elif filt is not None:
            entry, mid, ws_bytes = lib.wmf_recommend_topn_filtered, filt.upload(), lib.wmf_recommend_workspace_bytes
        else:
            entry, mid, ws_bytes = lib.wmf_recommend_topn, lambda b0: (), lib.wmf_recommend_workspace_bytes
        need = lambda rows: int(ws_bytes(rows, topn, 0))   # noqa: E731
        call = _topn_call(entry, (_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True)), self.items.shape[0], mid, topn, items_d, scores_d)
        return self._scan_batches(u, [None if seen is None else (seen.indptr, seen.indices)], need, [items_d, scores_d], call,
                                  self._windows(len(u), need) if wide else None)

    # ------------------------------------------------------------------ a14: similar_items, similar_users
    def similar_items(self, items, topn=10, metric='cosine', exclude_self=True, return_scores=False, allow=None, allow_idx=None):
        """The ``topn`` items closest to each of ``items`` in factor space (an int or a sequence of ints; negative indices count
        from the end), best first, equal scores in item order.  ``metric``: 'cosine' or 'dot', over the features -- the bias
        column of a bias model is not a feature in either.  ``exclude_self``: the item itself is not among its neighbours.
        One fused device pass over the catalogue per batch (wmf_similar_topn); a float64 model is served from its float32
        device copies, as ``recommend`` is.  The device copies hold both factor matrices, so the model must have its ``users``
        (an AttributeError otherwise, before the GPU is touched).  Arrays that ``train`` left behind are read-only: their copies
        and inverse norms are made once; with a writable array every call uploads both matrices and computes the norms again
        -- freeze the arrays (``a.flags.writeable = False``) when they no longer change.  Returns int64 [len(items), topn], padded with -1 where there are fewer rows; with
        ``return_scores`` also the float32 scores, padded with -inf.  An int gives one row.  ``topn`` is at most
        RECOMMEND_MAX_TOPN: there is no slower path beyond it, a larger ``topn`` is a ValueError.
        ``allow`` / ``allow_idx``: the neighbours are taken among the allowed rows only, given as for ``recommend`` (a bool mask
        of length items, a list of ids, or [G, items] masks with one ``allow_idx`` entry per query).  All three are served by the
        mask form (wmf_similar_topn_filtered): the scaled score has no list form, a list of ids becomes its mask.  The row
        itself is still left out under ``exclude_self`` when the mask allows it."""
        return self._similar("items", items, topn, metric, exclude_self, return_scores, allow, allow_idx)

    def similar_users(self, users, topn=10, metric='cosine', exclude_self=True, return_scores=False, allow=None, allow_idx=None):
        """``similar_items`` among the users: the ``topn`` users closest to each of ``users`` (masks of length users)."""
        return self._similar("users", users, topn, metric, exclude_self, return_scores, allow, allow_idx)

    def _similar(self, side, ids, topn, metric, exclude_self, return_scores, allow=None, allow_idx=None):
        if metric not in ('cosine', 'dot'):
            raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
        topn = int(topn)
        if topn < 1 or topn > RECOMMEND_MAX_TOPN:
            raise ValueError(f"topn must be between 1 and {RECOMMEND_MAX_TOPN}, not {topn}")
        if self.users is None:                                      # (the device copies are of both matrices; as in predict)
            raise AttributeError("the model has no user factors yet: train it, or assign users, before asking for neighbours")
        n_rows = getattr(self, side).shape[0]
        one = np.ndim(ids) == 0
        q = _wrapped_ids(np.atleast_1d(np.asarray(ids)).reshape(-1).astype(np.int64), n_rows, side[:-1], np.int64)
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_rows, len(q), side[:-1], as_mask=True)
        _lib.require_gpu()
        out_rows, out_scores = _padded(len(q), topn)
        if len(q) and not (filt is not None and filt.empty):
            self._similar_fused(side, q, topn, metric == 'cosine', bool(exclude_self), out_rows, out_scores if return_scores else None, filt)
        return _topn_result(out_rows, out_scores, one, return_scores)

    def _similar_fused(self, side, q, topn, cosine, exclude_self, out_rows, out_scores, filt=None):
        """wmf_similar_topn in batches (_scan_batches): the rows ``q`` of ``side`` against all of its rows.  ``filt``: an _Allow in
        the mask form, then wmf_similar_topn_filtered."""
        if cosine:
            users_t, items_t, f, ld, norms = self._device_inv_norms(side)
        else:
            users_t, items_t, f, ld = self._device_factors()
            norms = None
        mat = users_t if side == "users" else items_t
        lib = _lib.load()
        rows_d = torch.empty(len(q), topn, dtype=torch.int32, device="cuda")
        scores_d = torch.empty(len(q), topn, dtype=torch.float32, device="cuda") if out_scores is not None else None
        head = (_ptr(mat), _ptr(mat), f, ld, int(self.bias is True), _ptr(norms) if cosine else None, _ptr(norms) if cosine else None)
        own = (int(exclude_self), None, None)                      # (no exclusion lists: _scan_batches gets no CSR)
        if filt is None:
            entry, mid = lib.wmf_similar_topn, lambda b0: own
        else:
            at = filt.upload()
            entry, mid = lib.wmf_similar_topn_filtered, lambda b0: (*own, *at(b0)[:4])
        call = _topn_call(entry, head, mat.shape[0], mid, topn, rows_d, scores_d)
        out_rows[:], scores = self._scan_batches(q, [], lambda rows: lib.wmf_similar_workspace_bytes(rows, topn, 0), [rows_d, scores_d], call)
        if out_scores is not None:
            out_scores[:] = scores

    # ------------------------------------------------------------------ a12: rank_positions
    def rank_positions(self, test_mat, exclude=None, users=None, return_scores=False):
        """The exact place of every held-out item in the user's full-catalogue order: for each stored entry (u, t) of
        ``test_mat`` (stored zeros too) the number of items that ``u`` has no stored entry for in ``exclude`` and that
        ``recommend`` puts before ``t`` -- a higher score, or an equal score and a lower id -- so ``t`` is among
        ``recommend(u, k, exclude)`` exactly when ``0 <= rank < k``; -1 for a ``t`` that is itself in ``exclude``.  Both
        matrices are SciPy sparse of shape [users of the model, items]; they are canonicalised on copies (CSR, duplicates
        summed, indices sorted).  ``users``: the rows asked for (negative indices count from the end), default all rows
        with stored entries.  Returns ``(indptr, indices, ranks)`` -- the CSR structure of the canonicalised
        ``test_mat[users]`` and int64 ranks aligned with ``indices`` -- and with ``return_scores`` also the float32 scores.
        One counting pass over the catalogue per batch of rows (wmf_rank_positions); nothing is sampled."""
        u, test, seen = ranking_inputs(test_mat, exclude, users, (self.users.shape[0], self.items.shape[0]))
        _lib.require_gpu()
        indptr, indices = test.indptr.astype(np.int64), test.indices.astype(np.int64)
        ranks, scores = np.empty(len(indices), dtype=np.int64), np.empty(len(indices), dtype=np.float32)
        if len(indices):
            # a row of the device call holds at most RANKPOS_MAX_TARGETS targets: longer rows of test_mat become several
            per_user = np.diff(indptr)
            n_sub = -(-per_user // RANKPOS_MAX_TARGETS)
            owner = np.repeat(np.arange(len(u)), n_sub)            # the row of `test` a device row belongs to
            first = np.concatenate([[0], np.cumsum(n_sub)])[:-1]
            starts = indptr[owner] + RANKPOS_MAX_TARGETS * (np.arange(len(owner)) - first[owner])
            target_indptr = np.append(starts, indptr[-1]).astype(np.int64)
            seen_rows = seen[owner] if seen is not None else None
            r, s = self._rank_positions_fused(u[owner], target_indptr, indices, seen_rows, return_scores)
            ranks[:] = r
            if return_scores:
                scores[:] = s
        return (indptr, indices, ranks, scores) if return_scores else (indptr, indices, ranks)

    def _rank_positions_fused(self, u, target_indptr, target_indices, seen, want_scores):
        """wmf_rank_positions in batches (_scan_batches); returns [ranks, scores or None] aligned with ``target_indices``."""
        users_t, items_t, f, ld = self._device_factors()
        lib = _lib.load()
        rank_d = torch.empty(len(target_indices), dtype=torch.int32, device="cuda")
        score_d = torch.empty(len(target_indices), dtype=torch.float32, device="cuda") if want_scores else None
        # (the pointers index the whole output arrays, as they do the index arrays)
        return self._scan_batches(
            u, [None if seen is None else (seen.indptr, seen.indices), (target_indptr, target_indices)],
            lambda rows: lib.wmf_rank_positions_workspace_bytes(rows, len(target_indices), 0), [rank_d, score_d],
            lambda b0, nb, ids, csrs, *ws: lib.wmf_rank_positions(
                _ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True), ids, nb, self.items.shape[0], *csrs[0], *csrs[1], 0,
                _ptr(rank_d), _ptr(score_d) if want_scores else None, *ws))

    def _rank_positions(self, test_mat, exclude, users):
        """eval_ranking's exact ranks from the device: rank_positions."""
        return self.rank_positions(test_mat, exclude, users)

    def _hit_counts(self, pair_user, pair_item, pair_row, candidates, slot, topn):
        """compute_hit (base_model.py:51-98) for every test entry in one launch: wmf_hit_counts."""
        users_t, items_t, f, ld = self._device_factors()
        lib = _lib.load()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()   # noqa: E731
        pu, pi, pr, cd, sl, tn = dev(pair_user), dev(pair_item), dev(pair_row), dev(candidates), dev(slot), dev(topn)
        hits = torch.zeros(len(topn), dtype=torch.int64, device="cuda")
        _lib.check(lib.wmf_hit_counts(_ptr(users_t), _ptr(items_t), f, ld, int(self.bias is True), _ptr(pu), _ptr(pi), _ptr(pr),
                                      len(pair_user), _ptr(cd), candidates.shape[1], _ptr(sl), _ptr(tn), len(topn), _ptr(hits),
                                      _stream()))
        return hits.cpu().numpy()

    # ------------------------------------------------------------------ a8: eval_prec backend
    def _eval_sums(self, utility_mat):
        eng = self._engine
        if eng is None or not (eng.has_factors["users"] and eng.has_factors["items"]) or self._stale():
            eng = self._new_engine()
            eng.set_factors("users", self.users)
            eng.set_factors("items", self.items)
        shard = eng.make_eval_shard(*_csr_parts(utility_mat))
        return eng.eval_sums(shard)

    def _stale(self):
        """True when the public arrays are not (or may no longer be) what the engine holds."""
        if self.users is None or self.users.flags.writeable or self.items.flags.writeable:
            return True
        return getattr(self, "_synced", None) != (id(self.users), id(self.items))

    def _freeze(self):
        """The arrays handed out after training mirror device state: in-place edits would silently not reach predict /
        rank / eval_prec, so they are made read-only (an edit raises; assigning a fresh array works as in the reference)."""
        self.users.flags.writeable = False
        self.items.flags.writeable = False
        self._synced = (id(self.users), id(self.items))
        self._dev = None
        self._inv_norms = {}
        self._white = {}

    def _pull(self, eng, sides=("users", "items")):
        for s in sides:
            setattr(self, s, eng.get_factors(s).astype(self.dtype, copy=False))
        self._freeze()

    # ------------------------------------------------------------------ a13: objective and per-row backward errors
    def objective(self, count_mat, side="users", alpha=10, beta=1, pre_process_count='log'):
        """The function the half step of ``side`` minimises, on the model's factors as they stand: the implicit-feedback
        objective over ALL (user, item) pairs with the confidences ``train`` builds from ``count_mat`` (a copy is transformed
        as there, wmf_model.py:119-123; ``side="items"`` reads count_mat.T.tocsr(), :128), in float64 on the device.
        Returns {"loss", "all_pairs", "stored", "reg", "n_stored"}: loss = all_pairs + stored + reg, the square of the score over
        all pairs, the stored entries' correction and gamma |X|_F^2 of ``side``.  Without biases, loss + gamma |F|_F^2 of
        the other side is the same number from either side (the Hu-Koren-Volinsky objective)."""
        return self._audit(count_mat, side, alpha, beta, pre_process_count, False)

    def row_backward_errors(self, count_mat, side="users", alpha=10, beta=1, pre_process_count='log'):
        """For every row of ``side`` the normwise backward error of its normal equations A_u x_u = b_u (wmf_model.py:237-239 /
        :343-350) at the model's factors: |A_u x_u - b_u| / ((|G~ + gamma I|_F + a_u) |x_u| + |b_u|), float64 [n_side]; a row
        the half step solved to working precision is at the unit roundoff of the factors' dtype."""
        return self._audit(count_mat, side, alpha, beta, pre_process_count, True)

    def _audit(self, count_mat, side, alpha, beta, pre_process_count, rows):
        if self.weighted is not True:
            raise ValueError("the objective and the row systems are those of the weighted branch (weighted=True)")
        if side not in ("users", "items"):
            raise ValueError(f"side must be 'users' or 'items', not {side!r}")
        if pre_process_count not in ('log', 'linear'):
            raise ValueError(f"Pre_process_count {pre_process_count} is not implement please use log or linear.")
        if self.users is None:
            raise ValueError("the model has no user factors yet: train it first")
        shape = (self.users.shape[0], self.items.shape[0])
        if not scipy.sparse.issparse(count_mat) or count_mat.shape != shape:
            raise ValueError(f"count_mat must be a sparse matrix of shape {shape}, got {getattr(count_mat, 'shape', None)}")
        if self.users.shape[1] != self.items.shape[1]:
            raise ValueError(f"users and items have different widths: {self.users.shape[1]} and {self.items.shape[1]}")
        _lib.require_gpu()
        bias = self.bias is True
        mode = 0 if pre_process_count == 'log' else 1
        if self.users.dtype == np.float64 or self.items.dtype == np.float64:
            K = self._new_engine().K
            mat = scipy.sparse.csr_matrix(count_mat)
            mat = mat if side == "users" else mat.T.tocsr()
            fixed = "items" if side == "users" else "users"
            dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
            vals = dev(mat.data, np.float64)
            K.confidence_transform(vals, alpha, beta, mode)
            out = audit_f64(K, dev(getattr(self, side), np.float64), dev(getattr(self, fixed), np.float64), bias, float(self.gamma),
                            dev(mat.indptr, np.int64), dev(mat.indices, np.int32), vals, rows)
        else:
            eng = self._new_engine()
            eng.set_factors("users", self.users)
            eng.set_factors("items", self.items)
            indptr, indices, values = _csr_parts(count_mat)
            values = values.to(eng.device)
            eng.K.confidence_transform(values, alpha, beta, mode)
            eng.set_interactions(indptr, indices, values)
            out = eng.audit(side, rows)
        return out.pop("eta").cpu().numpy() if rows else out

    # ------------------------------------------------------------------ a15: explain
    def _device_whitening(self):
        """(users_t, items_t, f, ld, W_white of the item copy for the model's gamma): wmf_gram + wmf_factorize on the device copy
        of ``items``, kept exactly as long as that copy is (as ``_device_inv_norms``) and per gamma."""
        users_t, items_t, f, ld = dev = self._device_factors()
        key = float(self.gamma)
        if key not in self._white:
            lib = _lib.load()
            ws = torch.empty(int(lib.wmf_gram_workspace_bytes(f)), dtype=torch.uint8, device="cuda")
            G = torch.empty(f * f, dtype=torch.float64, device="cuda")
            W_white, W_unwhite = (torch.zeros(f, ld, dtype=torch.float32, device="cuda") for _ in range(2))
            info = torch.zeros(4, dtype=torch.int32, device="cuda")
            _lib.check(lib.wmf_gram(_ptr(items_t), items_t.shape[0], f, ld, int(self.bias is True), _ptr(G), _ptr(ws), _stream()))
            _lib.check(lib.wmf_factorize(_ptr(G), f, ld, key, _ptr(W_white), _ptr(W_unwhite), _ptr(info), _ptr(ws), _stream()))
            minor = int(info[0])
            if minor:
                raise _lib.WmfNumericError(f"Gramian + gamma*I is not positive definite (leading minor {minor})")
            self._white[key] = W_white
        return dev + (self._white[key],)

    def _row_system_head(self):
        """(head, items_t, f, ld): the leading arguments (Y, m, f, ld, bias, W_white) of the library's four calls on a row's own
        system -- wmf_explain_rows, wmf_foldin_rows, wmf_posterior_draw_rows, wmf_posterior_score_rows -- from _device_whitening."""
        _, items_t, f, ld, W_white = self._device_whitening()
        return (_ptr(items_t), items_t.shape[0], f, ld, int(self.bias is True), _ptr(W_white)), items_t, f, ld

    def explain(self, users, items, count_mat, topk=10, alpha=10, beta=1, pre_process_count='log'):
        """Why these items: the score of each of ``items`` for each of ``users`` with the user's row of ``count_mat`` folded in
        -- ``predict`` on ``recompute_factors[_bias](items, C_u, gamma)`` (wmf_model.py:213-240 / :311-351), which is the
        model's own score right after a user half step -- split into one term per stored entry of the user's history:
        contrib = (w_e + 1) y~_i^T A_u^-1 y~_j with the A_u of wmf_model.py:231-239 / :343-350, total = their sum + the item's
        bias.  With a bias model the user's bias is part of the folded-in row and so is shared out over the entries.
        ``users``: an int or a sequence of B ids (negative ids count from the end, as in ``recommend``).  ``items``: [B, T] or [B]
        item ids, for an int user a 1-D list of T items; -1 is an empty slot, so the output of ``recommend`` can be passed
        straight in.  ``count_mat``: the [users, items] count matrix of ``train``; the requested rows are read as stored and
        transformed on the device as ``train`` does (wmf_model.py:119-123).
        Returns, with ``topk`` set, ``(total float32 [B, T], history_items int64 [B, T, topk], contributions float32 [B, T,
        topk])``: the largest contributions first, equal ones in stored order, padded with -1 / 0.  With ``topk=None``:
        ``(total, indptr, indices, contributions [nnz, T])`` on the requested rows as stored.  An int user drops the B axis, 1-D
        ``items`` for a sequence of users drop the T axis.  A row whose system is not positive definite (effective weights
        <= -1) comes back as NaN.  One workgroup per row on the device (wmf_explain_rows); a float64 model is served from its
        float32 copies, as ``recommend`` is."""
        if self.weighted is not True:
            raise ValueError("the contributions are those of the weighted branch (weighted=True)")
        if pre_process_count not in ('log', 'linear'):
            raise ValueError(f"Pre_process_count {pre_process_count} is not implement please use log or linear.")
        if self.users is None:
            raise ValueError("the model has no user factors yet: train it first")
        n_users_model, n_items = self.users.shape[0], self.items.shape[0]
        if not scipy.sparse.issparse(count_mat) or count_mat.shape != (n_users_model, n_items):
            raise ValueError(f"count_mat must be a sparse matrix of shape {(n_users_model, n_items)}, got {getattr(count_mat, 'shape', None)}")
        if topk is not None and int(topk) < 1:
            raise ValueError(f"topk must be at least 1 or None, not {topk}")
        one = np.ndim(users) == 0
        u = _wrapped_ids(np.atleast_1d(np.asarray(users)).reshape(-1).astype(np.int64), n_users_model, "user", np.int64)
        flat = np.ndim(items) == 1 and not one

        def shaped(tg):
            if one and tg.ndim == 1:
                tg = tg.reshape(1, -1)
            elif flat and tg.shape[0] == len(u):
                tg = tg.reshape(-1, 1)
            if tg.ndim != 2 or tg.shape[0] != len(u) or tg.shape[1] < 1:
                raise ValueError(f"items must have shape [{len(u)}, T] or [{len(u)}] (an int user: [T]), got {np.shape(items)}")
            return tg
        tg = _target_ids(items, n_items, shaped)
        _lib.require_gpu()
        # the requested rows exactly as stored (stored zeros, duplicates and their order are kept)
        mat = count_mat if scipy.sparse.isspmatrix_csr(count_mat) else scipy.sparse.csr_matrix(count_mat)
        lens = (mat.indptr[u + 1] - mat.indptr[u]).astype(np.int64)
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pos = np.repeat(mat.indptr[u].astype(np.int64) - indptr[:-1], lens) + np.arange(indptr[-1], dtype=np.int64)
        indices = mat.indices[pos].astype(np.int64)
        B, T, nnz = len(u), tg.shape[1], int(indptr[-1])
        total = np.zeros((B, T), dtype=np.float32)
        contrib = np.zeros((nnz, T), dtype=np.float32)
        if B:
            self._explain_rows(u, indptr, indices, np.asarray(mat.data[pos], dtype=np.float32), tg, alpha, beta,
                               0 if pre_process_count == 'log' else 1, total, contrib)
        if topk is None:
            out = (total, indptr, indices, contrib)
            if one:
                out = (total[0],) + out[1:]
            elif flat:
                out = (total[:, 0], indptr, indices, contrib[:, 0])
            return out
        topk = int(topk)
        hist = np.full((B, T, topk), -1, dtype=np.int64)
        best = np.zeros((B, T, topk), dtype=np.float32)
        for b in range(B):
            lo, hi = indptr[b], indptr[b + 1]
            keep = min(topk, hi - lo)
            for t in np.nonzero(tg[b] >= 0)[0] if keep else ():
                order = np.argsort(-contrib[lo:hi, t], kind="stable")[:keep]      # largest first, equal ones in stored order
                hist[b, t, :keep] = indices[lo:hi][order]
                best[b, t, :keep] = contrib[lo:hi, t][order]
        out = (total, hist, best)
        if one:
            out = tuple(o[0] for o in out)
        elif flat:
            out = tuple(o[:, 0] for o in out)
        return out

    def _explain_rows(self, u, indptr, indices, counts, tg, alpha, beta, mode, total, contrib):
        """wmf_explain_rows in batches of rows (_scan_batches) and slices of at most EXPLAIN_MAX_TARGETS targets; fills ``total``
        [B, T] and ``contrib`` [nnz, T]."""
        head, _, f, _ = self._row_system_head()
        lib = _lib.load()
        vals = self._device_confidences(counts, alpha, beta, mode)
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t0 in range(0, tg.shape[1], EXPLAIN_MAX_TARGETS):
            part = np.ascontiguousarray(tg[:, t0: t0 + EXPLAIN_MAX_TARGETS], dtype=np.int32)
            tc = part.shape[1]
            tg_d = torch.from_numpy(part).cuda()
            total_d = torch.empty(len(u), tc, dtype=torch.float32, device="cuda")
            contrib_d = torch.empty(len(counts) + 1, tc, dtype=torch.float32, device="cuda")
            # (the pointers index the whole per-entry arrays, as they do the index array)
            total[:, t0: t0 + tc], got = self._scan_batches(
                u, [(indptr, indices)], lambda rows: lib.wmf_explain_workspace_bytes(rows, f, tc), [total_d, contrib_d],
                lambda b0, nb, ids, csrs, *ws: lib.wmf_explain_rows(
                    *head, *csrs[0], _ptr(vals), nb, _ptr(tg_d[b0:]), tc, _ptr(contrib_d), _ptr(total_d[b0:]), _ptr(fail), *ws))
            contrib[:, t0: t0 + tc] = got[:len(counts)]

    # ------------------------------------------------------------------ a16: fold_in, recommend_for
    def fold_in(self, count_rows, alpha=10, beta=1, pre_process_count='log'):
        """The factors of histories that need not be rows of the model: for each row of ``count_rows`` -- a SciPy sparse matrix
        of shape [B, items] for any B, e.g. the counts of new visitors, or of known users whose history has changed since
        ``train`` -- the row a user half step would give it against the model's items,
        ``recompute_factors[_bias](items, C, gamma)`` (wmf_model.py:213-240 / :311-351).  The rows are read as stored (stored
        zeros, duplicates and their order are kept) and transformed on the device as ``train`` transforms them
        (wmf_model.py:119-123).  Returns float32 [B, f], a block of rows of ``users``: with a bias model column 0 is the row's own
        bias.  An empty row gives zeros; a row whose system is not positive definite (effective weights <= -1) gives NaN.  One
        workgroup per row on the device (wmf_foldin_rows), from the whitening ``explain`` keeps: neither a whitened copy of the
        catalogue nor a plan is made.  A float64 model is served from its float32 copies, as ``recommend`` is."""
        mat, mode = self._foldin_arguments(count_rows, pre_process_count)
        f = self.items.shape[1]
        _lib.require_gpu()
        if mat.shape[0] == 0:
            return np.zeros((0, f), dtype=np.float32)
        X_d = self._fold_in_device(mat, alpha, beta, mode)[0]
        return np.ascontiguousarray(X_d[:, :f].cpu().numpy())

    def recommend_for(self, count_rows, topn=10, exclude_history=True, return_scores=False, alpha=10, beta=1,
                      pre_process_count='log', allow=None, allow_idx=None):
        """``recommend`` for histories instead of user ids: the rows of ``count_rows`` ([B, items], as for ``fold_in``) are
        folded in and the ``topn`` best items of the whole catalogue are found for each, best first, equal scores in item order;
        the factors never leave the device.  ``exclude_history``: the stored entries of a row (stored zeros too) are not
        recommended to it.  Returns int64 [B, topn], padded with -1 where a row has fewer eligible items; with ``return_scores``
        also the float32 scores, padded with -inf -- the items and scores of ``recommend`` on a model whose ``users`` are
        ``fold_in(count_rows)``, bit for bit.  A row whose fold-in failed (NaN factors) is all -1 / -inf.  ``topn`` is at most
        RECOMMEND_MAX_TOPN: a larger one is a ValueError.  ``allow`` / ``allow_idx``: the catalogue filter of ``recommend``
        (``allow_idx`` has one entry per row of ``count_rows``), with the same identity."""
        return self._recommend_for(count_rows, topn, RECOMMEND_MAX_TOPN, "topn", exclude_history, return_scores, alpha, beta,
                                   pre_process_count, allow, allow_idx)

    def candidates_for(self, count_rows, n=1000, exclude_history=True, return_scores=False, alpha=10, beta=1,
                       pre_process_count='log', allow=None, allow_idx=None):
        """``candidates`` for histories instead of user ids, as ``recommend_for`` is to ``recommend``: the rows of ``count_rows``
        are folded in on the device -- the factors never leave it -- and the ``n`` best items of the catalogue are found for each,
        1 <= n <= CANDIDATES_MAX (4096; a ValueError otherwise, before the GPU is asked for).  The arguments, padding and dtypes of
        ``recommend_for``; a row whose fold-in failed is all -1 / -inf.  Bit for bit the output of ``candidates`` on a model whose
        ``users`` are ``fold_in(count_rows)``."""
        return self._recommend_for(count_rows, n, CANDIDATES_MAX, "n", exclude_history, return_scores, alpha, beta, pre_process_count,
                                   allow, allow_idx)

    def recommend_diverse_for(self, count_rows, topn=10, pool=None, lam=0.7, metric='cosine', exclude_history=True, return_scores=False,
                              alpha=10, beta=1, pre_process_count='log', allow=None, allow_idx=None):
        """``recommend_diverse`` for histories instead of user ids, as ``recommend_for`` is to ``recommend``: the rows of
        ``count_rows`` are folded in on the device, their ``pool`` best items found (``candidates_for``) and re-ranked by greedy
        Maximal Marginal Relevance; neither the factors nor the pool leave the device.  The arguments of ``recommend_for`` and of
        ``recommend_diverse``; a row whose fold-in failed is all -1 / -inf.  Bit for bit the output of ``recommend_diverse`` on a
        model whose ``users`` are ``fold_in(count_rows)``."""
        topn, pool, lam, cosine = self._mmr_arguments(topn, pool, lam, metric)
        if pool < topn:
            raise ValueError(f"pool ({pool}) must be at least topn ({topn})")
        return self._recommend_for(count_rows, topn, RECOMMEND_MAX_TOPN, "topn", exclude_history, return_scores, alpha, beta,
                                   pre_process_count, allow, allow_idx, mmr=(pool, lam, cosine))

    def recommend_shelves_for(self, count_rows, groups, topn=10, exclude_history=True, return_scores=False, alpha=10, beta=1,
                              pre_process_count='log', allow=None, allow_idx=None, n_groups=None):
        """``recommend_shelves`` for histories instead of user ids, as ``candidates_for`` is to ``candidates``: the rows of
        ``count_rows`` are folded in on the device -- the factors never leave it -- and the ``topn`` best items of every shelf are
        found for each in one scan.  The arguments of ``recommend_for`` and of ``recommend_shelves``; returns int64 [B, G, topn]
        (and the float32 scores); a row whose fold-in failed is all -1 / -inf.  Bit for bit the output of ``recommend_shelves`` on
        a model whose ``users`` are ``fold_in(count_rows)``."""
        mat, mode = self._foldin_arguments(count_rows, pre_process_count)
        n_items = self.items.shape[0]
        g32, G, topn = self._shelf_arguments(groups, n_groups, topn, n_items)
        B = mat.shape[0]
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, n_items, B, "item", as_mask=True)
        _lib.require_gpu()
        out_items, out_scores = _padded(B, G, topn)
        if B and not (filt is not None and filt.empty):
            X_d, items_t, f, ld = self._fold_in_device(mat, alpha, beta, mode)
            seen = None
            if exclude_history:
                seen = mat.copy()                                  # the seen list as ``recommend`` prepares ``exclude``
                seen.sort_indices()
            got_items, got_scores = self._shelves_scan(X_d, items_t, f, ld, np.arange(B, dtype=np.int64), groups, g32, G, topn, seen,
                                                       return_scores, filt)
            good = ~torch.isnan(X_d[:, :f]).any(dim=1).cpu().numpy()
            out_items[good] = got_items[good]
            if return_scores:
                out_scores[good] = got_scores[good]
        return (out_items, out_scores) if return_scores else out_items

    # ------------------------------------------------------------------ a19: the posterior of a folded-in row
    def posterior_draws(self, count_rows, draws=1, sigma=1.0, seed=0, streams=None, alpha=10, beta=1, pre_process_count='log'):
        """Draws from the posterior of the folded-in rows: in the probabilistic reading of the row system of ``fold_in`` -- Gaussian
        likelihood, precision ``w + 1`` on a stored entry and 1 on every other item, prior precision ``gamma`` -- row u is
        ``N(x_u, A_u^-1)`` with ``x_u = fold_in(count_rows)[u]``, and each draw is ``x_u + sigma * A_u^-1/2 xi`` for standard normal
        ``xi`` (covariance ``sigma^2 A_u^-1``): wide for a visitor with three entries, narrow for one with three hundred.
        ``count_rows``, ``alpha``, ``beta``, ``pre_process_count`` as in ``fold_in``; 1 <= draws <= POSTERIOR_MAX_DRAWS, ``sigma``
        finite and >= 0, ``seed`` an integer in [0, 2^64), ``streams`` one unsigned integer per row (default: the row's position):
        a ValueError otherwise, before the GPU is asked for.  The noise is a pure function of (``seed``, the row's stream, the draw's
        number, the component): draw s of a row is the same whatever ``draws`` is and however the batch is cut, and the same
        (seed, stream) can serve ``sample_items_for`` as well.  Normal variates beyond 5.77 in size are never drawn.  Returns float32
        [B, draws, f]; ``sigma=0`` gives ``fold_in`` in every draw, bit for bit.  An empty row is drawn from the prior (zeros at
        ``sigma=0``); a row whose system is not positive definite gives NaN.  One workgroup per row on the device
        (wmf_posterior_draw_rows); a float64 model is served from its float32 copies."""
        mat, mode = self._foldin_arguments(count_rows, pre_process_count)
        draw = _Draw(draws, sigma, seed, streams, np.arange(mat.shape[0], dtype=np.uint64))
        f = self.items.shape[1]
        _lib.require_gpu()
        if mat.shape[0] == 0:
            return np.zeros((0, draw.draws, f), dtype=np.float32)
        X_d = self._fold_in_device(mat, alpha, beta, mode, draw)[0]
        return np.ascontiguousarray(X_d[:, :f].cpu().numpy()).reshape(mat.shape[0], draw.draws, f)

    def recommend_thompson_for(self, count_rows, topn=10, sigma=1.0, seed=0, streams=None, exclude_history=True, return_scores=False,
                               alpha=10, beta=1, pre_process_count='log', allow=None, allow_idx=None):
        """Thompson sampling for histories: ``recommend_for`` on ONE draw from each row's posterior (``posterior_draws`` with
        ``draws=1``) instead of on its mean -- the exploration of a factor model, proportionate to what the model does not know
        about the row.  The draw never leaves the device; the scores returned are the draw's.  The arguments of ``recommend_for`` and
        the ``sigma`` / ``seed`` / ``streams`` of ``posterior_draws``; ``topn`` up to CANDIDATES_MAX, beyond RECOMMEND_MAX_TOPN by
        the wide kernels, as in ``recommend``.  Bit for bit ``recommend`` on a model whose ``users`` are
        ``posterior_draws(count_rows, 1, ...)[:, 0]``; ``sigma=0`` is ``recommend_for``.  A failed row is all -1 / -inf."""
        mat, _ = self._foldin_arguments(count_rows, pre_process_count)
        draw = _Draw(1, sigma, seed, streams, np.arange(mat.shape[0], dtype=np.uint64))
        return self._recommend_for(mat, topn, CANDIDATES_MAX, "topn", exclude_history, return_scores, alpha, beta, pre_process_count,
                                   allow, allow_idx, draw=draw, wide=int(topn) > RECOMMEND_MAX_TOPN)

    def recommend_thompson(self, users, count_mat, topn=10, sigma=1.0, seed=0, streams=None, return_scores=False, alpha=10, beta=1,
                           pre_process_count='log', allow=None, allow_idx=None):
        """``recommend_thompson_for`` for trained ids: the rows ``count_mat[users]`` (``count_mat``: the [users, items] count matrix
        of ``train``), their stored entries excluded, and the default stream of a row its USER ID: the same user under the same seed
        gets the same list however the batch is cut.  An int user gives one row."""
        one, u = self._checked_users(users, count_mat)
        if count_mat is None:
            raise ValueError("count_mat must be the sparse [users, items] count matrix")
        rows = scipy.sparse.csr_matrix(count_mat)[u]
        out = self.recommend_thompson_for(rows, topn, sigma, seed, u.astype(np.uint64) if streams is None else streams, True, return_scores,
                                          alpha, beta, pre_process_count, allow, allow_idx)
        if one:
            out = tuple(o[0] for o in out) if return_scores else out[0]
        return out

    def score_posterior(self, count_rows, items, alpha=10, beta=1, pre_process_count='log'):
        """Mean and variance of the scores of ``items`` under the posterior of the folded-in rows (``posterior_draws``): ``items``
        int [B, T] for any T, -1 an empty slot -- the output of ``recommend_for`` can be passed straight in.  Returns ``(mean,
        var)``, float32 [B, T]: ``var = y~_i^T A_u^-1 y~_i``, never negative, the prior variance for an empty row; ``mean`` the
        score of the folded-in row, ``predict`` on ``fold_in(count_rows)`` up to rounding.  A -1 slot gives 0 in both, a row whose
        system is not positive definite NaN.  One workgroup per row (wmf_posterior_score_rows), POSTERIOR_MAX_TARGETS items a call."""
        mat, mode = self._foldin_arguments(count_rows, pre_process_count)
        B, n_items = mat.shape[0], self.items.shape[0]
        def shaped(tg):
            if tg.ndim != 2 or tg.shape[0] != B:
                raise ValueError(f"items must have shape [{B}, T], got {np.shape(items)}")
            return tg
        tg = _target_ids(items, n_items, shaped)
        _lib.require_gpu()
        mean, var = (np.zeros(tg.shape, dtype=np.float32) for _ in range(2))
        if tg.size:
            head, _, f, _ = self._row_system_head()
            lib = _lib.load()
            vals = self._device_confidences(mat.data, alpha, beta, mode)
            fail = torch.zeros(1, dtype=torch.int32, device="cuda")
            for t0 in range(0, tg.shape[1], POSTERIOR_MAX_TARGETS):
                tg_d = torch.from_numpy(np.ascontiguousarray(tg[:, t0: t0 + POSTERIOR_MAX_TARGETS], dtype=np.int32)).cuda()
                tc = tg_d.shape[1]
                mean_d, var_d = (torch.empty(B, tc, dtype=torch.float32, device="cuda") for _ in range(2))
                mean[:, t0: t0 + tc], var[:, t0: t0 + tc] = self._scan_batches(
                    np.arange(B, dtype=np.int64), [(mat.indptr, mat.indices)], lambda rows: lib.wmf_posterior_score_workspace_bytes(rows, f, tc),
                    [mean_d, var_d], lambda b0, nb, ids, csrs, *ws: lib.wmf_posterior_score_rows(
                        *head, *csrs[0], _ptr(vals), nb, _ptr(tg_d[b0:]), tc, _ptr(mean_d[b0:]), _ptr(var_d[b0:]), _ptr(fail), *ws))
        return mean, var

    def recommend_ucb_for(self, count_rows, topn=10, pool=None, c=1.0, exclude_history=True, return_scores=False, return_std=False,
                          alpha=10, beta=1, pre_process_count='log', allow=None, allow_idx=None):
        """Upper-confidence-bound re-ranking for histories: the ``pool`` best items of each folded-in row (``candidates_for``)
        re-ordered by ``score + c * std``, ``std`` the posterior standard deviation of the score (``score_posterior``), and the
        ``topn`` largest kept, equal keys to the lower id.  The pool, its scores and variances stay on the device
        (wmf_recommend_topn_wide into wmf_posterior_score_rows, per window of rows; the sort of at most 4096 float32 keys a row is
        torch's).  ``pool=None`` is ``min(10 * topn, CANDIDATES_MAX)``; 1 <= topn <= pool <= CANDIDATES_MAX, ``c`` finite and >= 0: a
        ValueError otherwise, before the GPU is asked for.  Returns the items int64 [B, topn], padded with -1; with ``return_scores``
        the MODEL's float32 scores (not the keys), padded with -inf; with ``return_std`` also the float32 standard deviations, 0 in
        the padding.  ``c=0`` is ``recommend_for``, bit for bit.  A failed row is all -1 / -inf / 0."""
        topn = int(topn)
        pool = min(10 * topn, CANDIDATES_MAX) if pool is None else int(pool)
        if pool < 1 or pool > CANDIDATES_MAX:
            raise ValueError(f"pool must be between 1 and {CANDIDATES_MAX}, not {pool}")
        if topn >= 1 and pool < topn:
            raise ValueError(f"pool ({pool}) must be at least topn ({topn})")
        cf = float(c)
        if not 0 <= cf <= float(np.finfo(np.float32).max):         # (a NaN fails the first)
            raise ValueError(f"c must be finite and >= 0, not {c!r}")
        return self._recommend_for(count_rows, topn, CANDIDATES_MAX, "topn", exclude_history, return_scores, alpha, beta, pre_process_count,
                                   allow, allow_idx, ucb=(pool, float(np.float32(cf)), bool(return_std)))

    def _ucb_scan(self, users_t, items_t, f, ld, u, topn, seen, filt, ucb, mat, vals):
        """``candidates`` re-ranked by score + c std without leaving the device: per window of _scan_batches,
        wmf_recommend_topn_wide(topn = pool) into pool buffers of one window's rows, wmf_posterior_score_rows on the pool as the
        rows' targets (the rows of ``mat``, ``vals`` its transformed values), and the two sorts -- by id, then stable and descending
        by key.  Returns the host (items, scores, std)."""
        pool, c, _ = ucb
        lib = _lib.load()
        head = self._row_system_head()[0]
        n_items = self.items.shape[0]
        need_scan = lambda rows: int(lib.wmf_recommend_wide_workspace_bytes(rows, pool, 0))   # noqa: E731
        need = lambda rows: max(need_scan(rows), int(lib.wmf_posterior_score_workspace_bytes(rows, f, pool)))   # noqa: E731
        rows = self._windows(len(u), need)
        pool_i = torch.empty(rows, pool, dtype=torch.int32, device="cuda")
        pool_s, pool_v = (torch.empty(rows, pool, dtype=torch.float32, device="cuda") for _ in range(2))
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        items_d = torch.empty(len(u), topn, dtype=torch.int32, device="cuda")
        scores_d, std_d = (torch.empty(len(u), topn, dtype=torch.float32, device="cuda") for _ in range(2))
        bias = int(self.bias is True)
        scan = _topn_call(lib.wmf_recommend_topn_wide, (_ptr(users_t), _ptr(items_t), f, ld, bias), n_items, _Allow.at(filt), pool, pool_i, pool_s,
                          moving=False)

        def call(b0, nb, ids, csrs, *ws):
            rc = scan(b0, nb, ids, csrs, *ws)
            if rc != _lib.WMF_OK:
                return rc
            rc = lib.wmf_posterior_score_rows(*head, *csrs[1], _ptr(vals), nb, _ptr(pool_i), pool, None, _ptr(pool_v), _ptr(fail), *ws)
            if rc != _lib.WMF_OK:
                return rc
            ids_sorted, by_id = torch.sort(pool_i[:nb], dim=1, stable=True)
            std = torch.sqrt(pool_v[:nb])
            key = pool_s[:nb] + c * std                            # (the padding: -inf + c * 0)
            order = torch.sort(key.gather(1, by_id), dim=1, descending=True, stable=True)[1][:, :topn]
            pick = by_id.gather(1, order)
            items_d[b0: b0 + nb] = pool_i[:nb].gather(1, pick)
            scores_d[b0: b0 + nb] = pool_s[:nb].gather(1, pick)
            std_d[b0: b0 + nb] = std.gather(1, pick)
            return _lib.WMF_OK
        return self._scan_batches(u, [None if seen is None else (seen.indptr, seen.indices), (mat.indptr, mat.indices)], need,
                                  [items_d, scores_d, std_d], call, rows)

    def _recommend_for(self, count_rows, topn, limit, name, exclude_history, return_scores, alpha, beta, pre_process_count, allow, allow_idx,
                       mmr=None, sample=None, draw=None, wide=None, ucb=None):
        """recommend_for (limit RECOMMEND_MAX_TOPN: the LDS kernels) and candidates_for (limit CANDIDATES_MAX: the wide ones);
        ``mmr``: the checked (pool, lam, cosine) of recommend_diverse_for (_diverse_scan); ``sample``: the _Sample of
        sample_items_for (_sample_scan), which also shapes the result; ``draw``: the _Draw (one draw a row) of
        recommend_thompson_for -- the rows are drawn instead of folded in; ``wide``: the wide kernels or not, where the limit does not
        say; ``ucb``: the checked (pool, c, return_std) of recommend_ucb_for (_ucb_scan), which adds the standard deviations."""
        mat, mode = self._foldin_arguments(count_rows, pre_process_count)
        topn = int(topn)
        if topn < 1 or topn > limit:
            raise ValueError(f"{name} must be between 1 and {limit}, not {topn}")
        B = mat.shape[0]
        filt = None if allow is None and allow_idx is None else _Allow(allow, allow_idx, self.items.shape[0], B, "item")
        _lib.require_gpu()
        out_items, out_scores = _padded(B, topn)
        out_std = np.zeros((B, topn), dtype=np.float32)
        want_scores = return_scores or (sample is not None and sample.want_logp)
        good = np.zeros(B, dtype=bool)
        if B and not (filt is not None and filt.empty):
            X_d, items_t, f, ld = self._fold_in_device(mat, alpha, beta, mode, draw)
            seen = None
            if exclude_history:
                seen = mat.copy()                                  # the seen list as ``recommend`` prepares ``exclude``
                seen.sort_indices()
            u = np.arange(B, dtype=np.int64)
            if ucb is not None:
                got_items, got_scores, got_std = self._ucb_scan(X_d, items_t, f, ld, u, topn, seen, filt, ucb, mat,
                                                                self._device_confidences(mat.data, alpha, beta, mode))
            else:
                got_items, got_scores = self._recommend_scan(X_d, items_t, f, ld, u, topn, seen, want_scores, filt,
                                                             limit == CANDIDATES_MAX if wide is None else wide, mmr, sample)
            good = ~torch.isnan(X_d[:, :f]).any(dim=1).cpu().numpy()
            out_items[good] = got_items[good]
            if want_scores:
                out_scores[good] = got_scores[good]
            if ucb is not None:
                out_std[good] = got_std[good]
        if sample is not None:
            return sample.result(out_items, out_scores, good, False, return_scores)
        if ucb is not None and ucb[2]:
            return (out_items, out_scores, out_std) if return_scores else (out_items, out_std)
        return (out_items, out_scores) if return_scores else out_items

    def _foldin_arguments(self, count_rows, pre_process_count):
        """The checks ``fold_in`` and ``recommend_for`` share, before the GPU is asked for; returns (the rows as CSR, as stored, and
        the transform's mode)."""
        if self.weighted is not True:
            raise ValueError("folding a history in is the half step of the weighted branch (weighted=True)")
        if pre_process_count not in ('log', 'linear'):
            raise ValueError(f"Pre_process_count {pre_process_count} is not implement please use log or linear.")
        if self.items is None or self.users is None:               # (the device copies are of both matrices; as in explain)
            raise ValueError("the model has no factors yet: train it, or assign users and items, before folding histories in")
        n_items = self.items.shape[0]
        if not scipy.sparse.issparse(count_rows) or count_rows.ndim != 2 or count_rows.shape[1] != n_items:
            raise ValueError(f"count_rows must be a sparse matrix of shape [B, {n_items}], got {getattr(count_rows, 'shape', None)}")
        mat = count_rows if scipy.sparse.isspmatrix_csr(count_rows) else scipy.sparse.csr_matrix(count_rows)
        return mat, 0 if pre_process_count == 'log' else 1

    @staticmethod
    def _device_confidences(counts, alpha, beta, mode):
        """The stored values ``counts`` of a CSR on the device, transformed as ``train`` transforms them (one spare element: never
        empty)."""
        vals = torch.from_numpy(np.append(np.asarray(counts, dtype=np.float32), np.float32(0))).cuda()
        _lib.check(_lib.load().wmf_confidence_transform(_ptr(vals), len(counts), float(alpha), float(beta), mode, _stream()))
        return vals

    def _fold_in_device(self, mat, alpha, beta, mode, draw=None):
        """wmf_foldin_rows in batches of rows (_scan_batches) on the rows of the CSR ``mat`` (at least one).  Returns (the folded
        block [B, ld] on the device in the library's layout, items_t, f, ld).  ``draw``: a _Draw, then wmf_posterior_draw_rows
        instead -- the block is [B * draw.draws, ld], the draws of a row next to each other, the streams' window moving with the
        rows'."""
        head, items_t, f, ld = self._row_system_head()
        lib = _lib.load()
        B = mat.shape[0]
        vals = self._device_confidences(mat.data, alpha, beta, mode)
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        if draw is None:
            X_d = torch.empty(B, ld, dtype=torch.float32, device="cuda")
            need = lambda rows: lib.wmf_foldin_workspace_bytes(rows, f)   # noqa: E731
            call = lambda b0, nb, ids, csrs, *ws: lib.wmf_foldin_rows(   # noqa: E731
                *head, *csrs[0], _ptr(vals), nb, _ptr(X_d[b0:]), _ptr(fail), *ws)
        else:
            D = draw.draws
            X_d = torch.empty(B * D, ld, dtype=torch.float32, device="cuda")
            streams_d = torch.from_numpy(draw.streams.view(np.int64)).cuda()
            need = lambda rows: lib.wmf_posterior_draw_workspace_bytes(rows, f, D)   # noqa: E731
            call = lambda b0, nb, ids, csrs, *ws: lib.wmf_posterior_draw_rows(   # noqa: E731
                *head, *csrs[0], _ptr(vals), nb, D, draw.sigma, draw.seed, _ptr(streams_d[b0:]), _ptr(X_d[b0 * D:]), _ptr(fail), *ws)
        self._scan_batches(np.arange(B, dtype=np.int64), [(mat.indptr, mat.indices)], need, [], call)
        return X_d, items_t, f, ld

    # ------------------------------------------------------------------ a3 / a4: operator seam
    def recompute_factors(self, Y, C, lambda_reg):
        """X_new for fixed factors Y and CSR C.  wmf_model.py:213-240 (host buffers in, host out)."""
        return self._recompute(Y, C, lambda_reg, 0)

    def recompute_factors_bias(self, Y, C, lambda_reg, cores=1):
        """Bias variant: column 0 of Y is the fixed side's bias.  wmf_model.py:311-351."""
        return self._recompute(Y, C, lambda_reg, 1)

    # ------------------------------------------------------------------ a5 / a6: the Pool variants
    def recompute_factors_par(self, Y, C, lambda_reg, cores=4):
        """wmf_model.py:242-250 (+ :289-309): the rows are independent, so `cores` has nothing to distribute here; what the
        variant changes is the dtype -- float64 rows stacked without a cast when Y or C is float64."""
        return self._recompute_par(Y, C, lambda_reg, 0)

    def recompute_factors_bias_par(self, Y, C, lambda_reg, cores=3):
        """wmf_model.py:252-265 (+ :267-287).  Column 0 of Y is the fixed side's bias (the caller's array is not modified)."""
        return self._recompute_par(Y, C, lambda_reg, 1)

    def _recompute_par(self, Y, C, lambda_reg, bias):
        C = scipy.sparse.csr_matrix(C)
        if np.result_type(np.asarray(Y).dtype, C.dtype) != np.float64:
            return self._recompute(Y, C, lambda_reg, bias)            # all-float32 inputs: float32 rows, as in the reference
        _lib.require_gpu()
        lib = _lib.load()
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        indptr = np.ascontiguousarray(C.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(C.indices, dtype=np.int32)
        values = np.ascontiguousarray(C.data, dtype=np.float64)
        X = np.empty((C.shape[0], Y.shape[1]), dtype=np.float64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _lib.check(lib.wmf_recompute_factors_f64_host(vp(Y), Y.shape[0], Y.shape[1], bias, vp(indptr), vp(indices),
                                                      vp(values), C.shape[0], float(lambda_reg), vp(X)))
        return X

    def _recompute(self, Y, C, lambda_reg, bias):
        _lib.require_gpu()
        lib = _lib.load()
        C = scipy.sparse.csr_matrix(C)
        if (np.result_type(np.asarray(Y).dtype, C.dtype) == np.float64 and C.nnz
                and float(np.nanmax(np.abs(C.data))) > F64_ROW_WEIGHT):
            # float64 row systems in the reference (:237-239), and weights beyond what the float32 kernels hold the tolerance
            # for: the float64 device path, rounded to the model's dtype where the reference rounds (:217)
            return self._recompute_par(np.asarray(Y, dtype=np.float64), C.astype(np.float64), lambda_reg, bias).astype(self.dtype)
        Y = np.ascontiguousarray(Y, dtype=np.float32)
        indptr = np.ascontiguousarray(C.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(C.indices, dtype=np.int32)
        values = np.ascontiguousarray(C.data, dtype=np.float32)
        X = np.empty((C.shape[0], Y.shape[1]), dtype=np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _lib.check(lib.wmf_recompute_factors_host(vp(Y), Y.shape[0], Y.shape[1], bias, vp(indptr), vp(indices),
                                                  vp(values), C.shape[0], float(lambda_reg), vp(X)))
        return X.astype(self.dtype, copy=False)

    # ------------------------------------------------------------------ a2: train
    def train(self, utility_mat, iterations, verbose=0, eval_mat=None, count_mat=None, alpha=10,
              cores=4, stopping_rounds=3, dtype='float64', min_improvement=0.0001,
              pre_process_count='log', beta=1, preprocess_mat=False, track_objective=False):
        """Alternating least squares with early stopping on eval MSE.  wmf_model.py:49-189.
        Returns the index of the last iteration run.  track_objective (weighted branch): ``self.objective_history`` gets one
        {"iteration", "users", "items"} per iteration -- the objective of each half step right after it (``objective``)."""
        utility_mat = utility_mat.copy()
        if count_mat is not None:
            count_mat = count_mat.copy()
        if self.bias is True and self.weighted is False:
            print("Bias computation is only implemented for weighted matrix factorization.")
        if eval_mat is None and verbose > 1:
            print("Since no explicit evaluation was provided the train matrix is used for evaluation.")
            eval_mat = utility_mat
        if preprocess_mat == True:  # noqa: E712  (the reference compares with ==)
            if pre_process_count == 'log':
                utility_mat.data = alpha * np.log(1 + beta * utility_mat.data)
            elif pre_process_count == 'linear':
                utility_mat.data = alpha * utility_mat.data

        eng = self._engine = self._new_engine()
        eng.set_factors("items", self.items)
        last_mse = - np.inf
        count_improvement = 0

        if self.weighted is not True:
            # closed-form un-weighted branch, wmf_model.py:73-115
            if self.bias is True:
                raise ValueError("operands could not be broadcast together: the un-weighted branch has no bias column")
            eng.set_interactions(*_csr_parts(utility_mat))
            eval_shard = self._train_eval_shard(eng, eval_mat)
            train_shard = eng.make_eval_shard(*_csr_parts(utility_mat)) if verbose > 1 else None
            for iter in range(iterations):
                if verbose > 0:
                    print(f"Starting fitting iteration {iter}")
                eng.half_step_unweighted("users")
                eng.half_step_unweighted("items")
                eng.check_numerics()
                mse_eval = self._mse(eng, eval_shard)
                if verbose > 0:
                    print(f"Current eval mse is {mse_eval}")
                if verbose > 1:
                    print(f"\tMSE Eval: {mse_eval}")
                    print(f"\tMSE Train: {self._mse(eng, train_shard)}")
                if mse_eval * (1 + min_improvement) > last_mse:
                    count_improvement += 1
                else:
                    count_improvement = 0
                last_mse = mse_eval
                if count_improvement >= stopping_rounds:
                    break
            self._pull(eng)
            # (the reference's dense-times-sparse products, :85 / :88, take NumPy's result type of the model dtype and the
            # utility matrix's: float64 for SciPy's default float64 matrices, float32 for float32 ones)
            out_dt = np.result_type(np.dtype(self.dtype), utility_mat.dtype)
            self.users, self.items = self.users.astype(out_dt), self.items.astype(out_dt)
            self._freeze()
            if verbose > 0:
                print("Training was completed.")
            if verbose > 1:
                print(f"MSE Eval at iteration {iter}: {self._mse(eng, eval_shard)}")
                print(f"MSE Train at iteration {iter}: {self._mse(eng, train_shard)}")
            return iter

        # weighted branch, wmf_model.py:116-189
        if pre_process_count not in ('log', 'linear'):
            raise ValueError(f"Pre_process_count {pre_process_count} is not implement please use log or linear.")
        if not cores >= 1:
            raise ValueError(f"Values of cores has to be positive not {cores}")
        if self.bias is not True and self.bias is not False:
            raise ValueError(f"self.bias = {self.bias} is unknown. Only True / False are allowed.")
        # cores > 1 with a float64 OR INTEGER count matrix: the reference's Pool variants keep float64 rows (:242-265) -- the
        # confidence transform of integer counts is float64 ('log', :120) or int64 ('linear', :123; the row products then
        # promote) -- so its training continues on float64 factors: the float64 device path then does the half steps, the
        # engine only the MSE (and builds neither float32 shards nor row plans).  float32 / float16 counts stay float32.
        # Which arithmetic the reference's rows run in: NumPy's result type of the factors and the TRANSFORMED counts
        # (np.log of int16 is float32, of int64 float64; alpha * int64 stays int64 and promotes with the float32 factors).
        tdt = _transformed_dtype(count_mat.dtype, alpha, beta, pre_process_count)
        rows64 = np.result_type(np.dtype(self.dtype), tdt) == np.float64
        f64 = None
        if rows64 and (cores > 1 or np.dtype(self.dtype) == np.float64):
            # (float64 factors: the Pool variants stack float64 rows, :242-265; a float64 model stores what it solves, :217)
            f64 = _Float64Steps(self, eng, count_mat, alpha, beta, pre_process_count)
        elif rows64 and count_mat.nnz and self._max_weight(count_mat, alpha, beta, pre_process_count) > F64_ROW_WEIGHT:
            # cores = 1: float64 rows, float32 factors (:217); the float32 kernels hold the tolerance up to F64_ROW_WEIGHT only
            f64 = _Float64Steps(self, eng, count_mat, alpha, beta, pre_process_count, store_float32=True)
        else:
            indptr, indices, values = _csr_parts(count_mat)
            values = values.to(eng.device)
            eng.K.confidence_transform(values, alpha, beta, 0 if pre_process_count == 'log' else 1)
            eng.set_interactions(indptr, indices, values)      # also builds the item-major shard (:128)
        eval_shard = self._train_eval_shard(eng, eval_mat)
        train_shard = eng.make_eval_shard(*_csr_parts(utility_mat)) if verbose > 1 else None

        for iter in range(iterations):
            if verbose > 0:
                print(f"Starting fitting iteration {iter}")
            start = time.time()
            if track_objective:
                if iter == 0:
                    self.objective_history = []
                track = {"iteration": iter}
                if f64 is not None:
                    f64.iteration(track)
                else:
                    for side in ("users", "items"):
                        eng.half_step(side)
                        track[side] = eng.audit(side)
                    eng.check_numerics()
                self.objective_history.append(track)
            elif f64 is not None:
                f64.iteration()
            else:
                eng.half_step("users")
                eng.half_step("items")
                eng.check_numerics()
            if self.bias is True and cores == 1:
                print(f"Iteration {iter} took {round(time.time() - start, 4)} seconds.")
            mse_eval = self._mse(eng, eval_shard)
            if mse_eval * (1 + min_improvement) > last_mse:
                count_improvement += 1
            else:
                count_improvement = 0
            last_mse = mse_eval
            if verbose > 0:
                print(f"Current eval mse is {mse_eval}")
            if verbose > 1:
                print(f"\tMSE Eval: {mse_eval}")
                print(f"\tMSE Train: {self._mse(eng, train_shard)}")
            if count_improvement >= stopping_rounds:
                break
        if f64 is not None:
            self.users, self.items = f64.factors()          # float64, as the reference's Pool variants leave them (float32 for cores = 1)
            self._freeze()
        else:
            self._pull(eng)
        if verbose > 0:
            print("Training was completed.")
        if verbose > 1:
            print(f"MSE Eval at iteration {iter}: {self._mse(eng, eval_shard)}")
            print(f"MSE Train at iteration {iter}: {self._mse(eng, train_shard)}")
        return iter

    @staticmethod
    def _max_weight(count_mat, alpha, beta, pre_process_count):
        """Largest confidence weight in magnitude the transform (wmf_model.py:119-123) gives this count matrix."""
        data = np.asarray(count_mat.data, dtype=np.float64)
        with np.errstate(all="ignore"):
            w = alpha * np.log(1 + beta * data) if pre_process_count == 'log' else alpha * data
        return float(np.nanmax(np.abs(w))) if w.size else 0.0

    @staticmethod
    def _train_eval_shard(eng, eval_mat):
        if eval_mat is None:
            # the reference fails inside eval_prec here (wmf_model.py:61-63 only substitutes when verbose > 1)
            raise AttributeError("'NoneType' object has no attribute 'nonzero'")
        return eng.make_eval_shard(*_csr_parts(eval_mat))

    @staticmethod
    def _mse(eng, shard):
        sq, _, cnt = eng.eval_sums(shard)
        return sq / cnt if cnt else float('nan')
