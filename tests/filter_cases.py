"""What the tests of the filtered catalogue scans share (tests/test_gpu_recommend_filtered.py, tests/test_recommend_filtered_cpu.py):
the allow-mask patterns, their packing into the words of include/wmf_hip.h, the reference route -- tests/recommend_ref.py with the
ineligible items added to the row's seen list -- and the plumbing to wmf_recommend_topn_filtered.  Importing it touches no GPU."""
import numpy as np

import recommend_ref as rref
import serving_ref as ref

PATTERNS = ("everything", "nothing", "item 0", "last item", "one tile", "all but one tile", "every other", "word edges",
            "without the 50 best", "random 30%", "random 1%", "dead bits set")
WORD_EDGES = (31, 32, 63, 64)
SENTINEL = -12345.0


def mask_row(pattern, rng, scores, seen, n):
    """The allow mask (bool [n]) of one row: `scores` the row's reference scores, `seen` its seen ids."""
    name = PATTERNS[pattern]
    m = np.zeros(n, dtype=bool)
    if name in ("everything", "dead bits set"):
        m[:] = True
    elif name == "item 0":
        m[0] = True
    elif name == "last item":
        m[n - 1] = True
    elif name in ("one tile", "all but one tile"):
        t = int(rng.integers(0, (n + 15) // 16))
        m[16 * t: 16 * t + 16] = True
        if name == "all but one tile":
            m = ~m
    elif name == "every other":
        m[::2] = True
    elif name == "word edges":
        m[[j for j in WORD_EDGES if j < n]] = True
    elif name == "without the 50 best":
        m[:] = True
        m[rref.recommend_ref(scores[:n], seen, 50)] = False         # the threshold has to be found far down
    elif name == "random 30%":
        m = rng.random(n) < 0.3
    elif name == "random 1%":
        m = rng.random(n) < 0.01
    return m


def mask_rows(pattern, rng, user_scores, seen, n):
    """[rows, n]: one mask per batch position."""
    return np.stack([mask_row(pattern, rng, s, [] if seen is None else seen[b], n) for b, s in enumerate(user_scores)])


def pack(masks, dead_bits=False):
    """bool [G, n] -> uint32 [G, ceil(n / 32)], item j at bit j & 31 of word j >> 5; dead_bits: the bits past n set too."""
    masks = np.atleast_2d(masks)
    G, n = masks.shape
    words = (n + 31) // 32
    bits = np.full((G, 32 * words), bool(dead_bits))
    bits[:, :n] = masks
    out = np.zeros((G, words), dtype=np.uint32)
    for k in range(32):
        out |= bits[:, k::32].astype(np.uint32) << np.uint32(k)
    return out


def unpack(words, n):
    """The inverse of pack on the first n bits."""
    words = np.atleast_2d(words)
    j = np.arange(n)
    return ((words[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def filtered_ref(scores, seen, mask, topn):
    """The reference route: the complement of the mask goes into the seen list of tests/recommend_ref.py."""
    return rref.recommend_ref(scores, np.concatenate([np.asarray(seen, dtype=np.int64), np.flatnonzero(~mask)]), topn)


def brute_force(scores, seen, mask, topn):
    """The topn best eligible unseen items by a plain sort on (-score, id), no shared code with recommend_ref."""
    elig = [j for j in range(len(scores)) if mask[j] and j not in set(int(s) for s in seen)]
    return np.array(sorted(elig, key=lambda j: (-scores[j], j))[:topn], dtype=np.int64)


class Filtered:
    """wmf_recommend_topn_filtered on one user list and one item matrix (tests/test_gpu_recommend.py's _Recommend with a filter)."""

    def __init__(self, Uf, If, f, ld, bias, user_idx):
        from scan_cases import _dev
        self.Ud, self.Id, self.args = _dev(ref.padded(Uf, ld)), _dev(ref.padded(If, ld)), (f, ld, bias)
        self.user_idx = _dev(user_idx, np.int32)
        self.n_users, self.n_items = len(user_idx), len(If)

    def __call__(self, topn, n_slices, seen=None, bits=None, allow_idx=None, cand=None, n_users=None, n_items=None, expect=None, **over):
        """bits: uint32 [G, words] (mask form); cand: ids (list form); over: allow_words / n_masks / n_cand / ws_bytes as passed."""
        import torch
        from scan_cases import _api, _dev
        _lib, lib, _ptr, _stream = _api()
        f, ld, bias = self.args
        nu, ni = n_users or self.n_users, n_items or self.n_items
        ws = torch.empty(int(lib.wmf_recommend_workspace_bytes(nu, max(topn, 1), n_slices)), dtype=torch.uint8, device="cuda")
        items = torch.full((nu + 2, topn), -7, dtype=torch.int32, device="cuda")        # a sentinel row on either side
        sc = torch.full((nu + 2, topn), SENTINEL, dtype=torch.float32, device="cuda")
        cnt = torch.full((nu + 2,), -7, dtype=torch.int32, device="cuda")
        ip_d = idx_d = bits_d = ai_d = cand_d = None
        if seen is not None:
            indptr, indices = rref.csr_of(seen)
            assert len(indptr) == nu + 1
            ip_d, idx_d = _dev(indptr, np.int64), _dev(indices, np.int32)
        words = n_masks = n_cand = 0
        if bits is not None:
            bits = np.atleast_2d(bits)
            bits_d, (n_masks, words) = _dev(bits.view(np.int32)), bits.shape
        if allow_idx is not None:
            ai_d = _dev(allow_idx, np.int32)
        if cand is not None:
            cand_d, n_cand = _dev(np.append(cand, 0), np.int32), len(cand)
        rc = lib.wmf_recommend_topn_filtered(_ptr(self.Ud), _ptr(self.Id), f, ld, bias, _ptr(self.user_idx), nu, ni, _ptr(ip_d), _ptr(idx_d),
                                             _ptr(bits_d), over.get("allow_words", words), over.get("n_masks", n_masks), _ptr(ai_d), _ptr(cand_d),
                                             over.get("n_cand", n_cand), topn, n_slices, _ptr(items[1:]), _ptr(sc[1:]), _ptr(cnt[1:]), _ptr(ws),
                                             over.get("ws_bytes", ws.numel()), _stream())
        items, sc, cnt = items.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
        for a, fill in ((items, -7), (sc, np.float32(SENTINEL)), (cnt, -7)):
            assert (a[0] == fill).all() and (a[-1] == fill).all(), "a sentinel around the outputs was written"
        if expect is not None:
            assert rc == expect, (rc, lib.wmf_last_error())
            assert (items == -7).all() and (sc == np.float32(SENTINEL)).all() and (cnt == -7).all(), "a refused call wrote its outputs"
            return None
        _lib.check(rc)
        return items[1:-1], sc[1:-1], cnt[1:-1]


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def case_rows(f, bias, cls, pattern):
    """(users, seen rows, masks [N_USERS, N_ITEMS]) of one pattern at one width and input class: the rows the GPU test sends and the
    CPU test holds to account.  The seen-row patterns of tests/scan_cases.py turn with the mask pattern."""
    from scan_cases import N_ITEMS, _scores, _seen_rows, _user_list
    rng = np.random.default_rng(7000 + 100 * pattern + 2 * f + bias)
    users = _user_list()
    S = _scores(f, bias, cls)[0]
    seen = _seen_rows(rng, S[users], N_ITEMS, pattern)
    return users, seen, mask_rows(pattern, rng, S[users], seen, N_ITEMS)


def bits_of(pattern, masks):
    """(uint32 masks, allow_idx) as a call sends them: one mask and allow_idx NULL where every row has the same mask, else a mask per
    batch position."""
    dead = PATTERNS[pattern] == "dead bits set"
    if (masks == masks[0]).all():
        return pack(masks[:1], dead), None
    return pack(masks, dead), np.arange(len(masks))
