"""Host-side reference of the sampled top-n (include/wmf_hip.h, wmf_sample_topn / wmf_sample_noise / wmf_log_partition), in plain
NumPy: the hash in uint64, u and g in float64, the sampled list of a row given its scores and its noise, the Plackett-Luce
probabilities the chi-square tests hold the draws to, and a float64 log-sum-exp.  Nothing here touches a GPU:
tests/test_sample_cpu.py checks it against a brute-force loop."""
import numpy as np

import recommend_ref as rref

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
K_MAX = 2 ** 23 - 1
G_MIN, G_MAX = -2.8116, 16.6356                                     # the range the header states


def mix(z):
    """uint64 -> uint64, wrapping: the finaliser of the header."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def noise_k(seed, streams, items):
    """The 23 bits of every (stream, item) pair, broadcast: uint32.  `items` are 32-bit ids, zero-extended."""
    streams = np.asarray(streams, dtype=np.uint64)
    items = np.asarray(items, dtype=np.int64).astype(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        a = mix(np.uint64(seed) + GOLDEN * (streams + np.uint64(1)))
        h = mix(a + GOLDEN * (items + np.uint64(1)))
    return (h >> np.uint64(41)).astype(np.uint32)


def noise_u(k):
    """(2 k + 1) 2^-24 in float64 (exact there and in float32)."""
    return (2.0 * np.asarray(k, dtype=np.float64) + 1.0) * 2.0 ** -24


def noise_g(k):
    """-log(-log(u)) in float64."""
    return -np.log(-np.log(noise_u(k)))


def noise_matrix(seed, streams, n_items):
    """float64 [len(streams), n_items]: g of every (stream, item)."""
    return noise_g(noise_k(seed, np.asarray(streams, dtype=np.uint64)[:, None], np.arange(n_items)[None, :]))


def perturbed_exact(scores, temperature, g32):
    """float32 z = the correctly rounded exact scores + temperature * g32, for integer scores below 2^12, a power of two temperature
    and float32 noise: the sum spans fewer than 64 bits, so np.longdouble (64-bit significand) holds it exactly and the cast rounds
    once, as the device's fmaf does."""
    assert np.finfo(np.longdouble).nmant >= 63 and np.abs(scores).max(initial=0) < 2 ** 12 and np.log2(temperature) % 1 == 0
    g32 = np.asarray(g32)
    assert g32.dtype == np.float32
    exact = np.asarray(scores).astype(np.longdouble) + np.longdouble(temperature) * g32.astype(np.longdouble)
    return exact.astype(np.float32)


def sample_row(z, seen, n):
    """The list of one row: its n largest z among the items not in `seen`, largest first, equal z (-0.0 is +0.0) to the lower id."""
    return rref.recommend_ref(np.asarray(z, dtype=np.float64), seen, n)


def sample_lists(scores, noise, temperature, seen, n):
    """One list per row of `scores` (float64 [B, n_items]) under `noise` of the same shape: z = scores + temperature * noise in
    float64."""
    z = np.asarray(scores, dtype=np.float64) + float(temperature) * np.asarray(noise, dtype=np.float64)
    return [sample_row(z[b], [] if seen is None else seen[b], n) for b in range(len(z))]


def plackett_luce_first(scores, temperature):
    """P(item i is drawn first) = softmax(scores / temperature)."""
    x = np.asarray(scores, dtype=np.float64) / temperature
    p = np.exp(x - x.max())
    return p / p.sum()


def plackett_luce_pairs(scores, temperature):
    """P(i first, j second) = p_i p_j / (1 - p_i): float64 [n, n], zero on the diagonal."""
    p = plackett_luce_first(scores, temperature)
    P = p[:, None] * p[None, :] / (1.0 - p[:, None])
    np.fill_diagonal(P, 0.0)
    return P


def chi_square(observed, expected, floor=5.0):
    """(statistic, cells) over the cells whose expectation is at least `floor`."""
    observed, expected = np.asarray(observed, dtype=np.float64).ravel(), np.asarray(expected, dtype=np.float64).ravel()
    keep = expected >= floor
    return float(((observed[keep] - expected[keep]) ** 2 / expected[keep]).sum()), int(keep.sum())


def logsumexp64(x):
    """log sum exp of a float64 vector; -inf for none."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0 or x.max() == -np.inf:
        return -np.inf
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))
