"""Timing lab for the dense shared-work kernels on a real GPU (not a test): Gramian and row transform of an [m, f] factor
block.  Usage: python tools/dense_lab.py m k bias reps [flags,...]
(flags: numbers or names, e.g. 0,F32_GRAM; recmodel_amd/_lib.py DEBUG_FLAGS)
A library with the chained whitening (wmf_chained_supported) is also timed on it: the Gramian of g and the chained pass with a
dense and with an anti-triangular N_ext, next to the Gramian, the whitening and the un-whitening they replace.  WMF_HIP_LIB
names the library (recmodel_amd/_lib.py): two runs, one per library, are an A/B."""
import sys
import torch
sys.path.insert(0, '.')
from recmodel_amd import _lib
from recmodel_amd.engine import HipKernels

m = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
k = int(sys.argv[2]) if len(sys.argv) > 2 else 128
bias = int(sys.argv[3]) if len(sys.argv) > 3 else 1
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
flags = [_lib.parse_debug_flags(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "0").split(",")]
lib = _lib.load()
K = HipKernels()
f = k + (2 if bias else 0) - (1 if bias else 0)            # the engine's f: k + 1 with biases
ld = K.ld_for(f)
dev = torch.device("cuda")
torch.manual_seed(5)
X = torch.rand(m, ld, device=dev) * 0.1
X[:, f:] = 0
G = torch.zeros(f, f, dtype=torch.float64, device=dev)
ws = torch.empty(K.gram_workspace_bytes(f), dtype=torch.uint8, device=dev)
W = torch.triu(torch.randn(f, ld, device=dev) * 0.05)          # (the whitening matrices are triangular)
ldv = K.whitened_row_floats(f, ld, bias)
V = torch.empty(m, ldv, device=dev)
pairs = torch.empty(m, 2, device=dev) if (bias and ldv != ld) else torch.empty(m, device=dev)
out2 = torch.empty(m, ld, device=dev)
Gref = None
for fl in flags:
    _lib.check(lib.wmf_debug_set_flags(fl))
    lib.wmf_profile_enable(0)
    K.gram(X, m, f, ld, bias, G, ws)
    K.row_transform(X, m, f, ld, W, bias, V, pairs if bias else None)
    K.row_transform(X, m, f, ld, W, False, out2, None)
    torch.cuda.synchronize()
    lib.wmf_profile_enable(1)
    for _ in range(reps):
        K.gram(X, m, f, ld, bias, G, ws)
        K.row_transform(X, m, f, ld, W, bias, V, pairs if bias else None)
        K.row_transform(X, m, f, ld, W, False, out2, None)
    torch.cuda.synchronize()
    lib.wmf_profile_enable(0)
    print(f"flags={fl}: " + ", ".join(f"{nm}={ms / max(n, 1):.3f}ms x{n // reps}" for nm, _, ms, n, _, _ in _lib.profile_table(lib)))
    lib.wmf_profile_reset()
    if Gref is None:
        Gref = G.clone()
        G64 = (X[:1_000_000, :f].double().T @ X[:1_000_000, :f].double()) if not bias else None
    else:
        print(f"    gram vs flags={flags[0]}: {float((G - Gref).abs().max() / Gref.abs().max()):.2e}")
lib.wmf_debug_set_flags(0)

# ---- the chained whitening: gram_whitened + row_transform_chained on g against gram + whitening + un-whitening ----
if hasattr(K, "chained_supported") and K.chained_supported(f, ld, bias):
    rolled = bool(bias and ldv != ld and K.rolled_layout_supported(f, ld))
    f1 = f + (1 if bias else 0)
    ws1 = torch.empty(K.gram_workspace_bytes(f + 1), dtype=torch.uint8, device=dev)
    Gaug = torch.zeros(f1 * f1, dtype=torch.float64, device=dev)
    N = torch.zeros(f1, ld, device=dev)
    N[:, :f1] = torch.randn(f1, f1, device=dev) * 0.05          # dense: a lower- times an upper-triangular matrix
    # ... and anti-triangular, as the engine's is with the users' whitening reversed: zero for i + j < f in
    # feature indices (f - 1 without biases), here in the kernel's positions
    pos = torch.cat([(torch.arange(f) + 1) % f, torch.arange(f, f1)]) if rolled else torch.arange(f1)
    N_dense, N_anti = N.clone(), N.clone()
    N_anti[:, :f1][(pos[:, None] + pos[None, :] < (f if bias else f - 1)).to(dev)] = 0
    nfb = (f1 + 15) // 16
    nkc = (16 * nfb + 31) // 32

    def live_pairs(M):
        """(32-wide K chunk, 16-wide output block) tiles of N_ext that are not all zero, and how many of them lie in a last
        chunk of one or two live positions (a library that starts the accumulators from that chunk issues none of those)."""
        P = torch.zeros(32 * nkc, 16 * nfb, device=dev)
        P[:f1, :f1] = M[:, :f1]
        live = (P.reshape(nkc, 32, nfb, 16) != 0).any(3).any(1)
        return int(live.sum()), int(live[-1].sum()) if f1 - 32 * (nkc - 1) <= 2 else 0
    Wl = torch.tril(torch.randn(f, ld, device=dev) * 0.05)
    Wl[:, f:] = 0

    def chained_trip():
        K.gram_whitened(X, m, f, ld, bias, Gaug, ws1)
        K.row_transform_chained(X, m, f, ld, bias, N, rolled, V, pairs if bias else None)

    def eager_trip():
        K.row_transform(X, m, f, ld, Wl, 4 if rolled else False, out2, None)
        K.gram(out2, m, f, ld, bias, G, ws)
        K.row_transform(out2, m, f, ld, W, (3 if rolled else bias), V, pairs if bias else None)

    # (the two shapes of N_ext alternate, twice: the order is not what is measured)
    for name, trip, M in (("eager", eager_trip, None),) + (("chained, dense N_ext", chained_trip, N_dense),
                                                          ("chained, anti-triangular N_ext", chained_trip, N_anti)) * 2:
        if M is not None:
            N.copy_(M)
            name += " (live tile pairs %d, %d of them in a short last chunk)" % live_pairs(M)
        trip()
        torch.cuda.synchronize()
        lib.wmf_profile_enable(1)
        for _ in range(reps):
            trip()
        torch.cuda.synchronize()
        lib.wmf_profile_enable(0)
        tab = _lib.profile_table(lib)
        print(f"{name} (rolled={int(rolled)}): " + ", ".join(f"{nm}={ms / max(n, 1):.3f}ms [{lo:.3f} .. {hi:.3f}] x{n // reps}" for nm, _, ms, n, lo, hi in tab)
              + f"; sum per trip {sum(ms for _, _, ms, _, _, _ in tab) / reps:.3f} ms")
        lib.wmf_profile_reset()
