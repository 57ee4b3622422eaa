"""The noise of central DP-FedAvg restated in numpy (kernel ``k_gaussian_noise``,
fedn_amd/csrc/dp_noise.h): the deviate of element ``i`` is a pure function of ``(seed, stream_id, round_id, i)``.

    (x0, x1, x2, x3) = Philox4x32-10(ctr = (i mod 2^32, i >> 32, stream_id, round_id), key = (seed mod 2^32, seed >> 32))
    u1 = ((x0 >> 5) * 2^26 + (x1 >> 6) + 1) * 2^-53        in (0, 1]
    u2 = ((x2 >> 5) * 2^26 + (x3 >> 6)) * 2^-53            in [0, 1)
    z  = sqrt(-2 * log(u1)) * cos(TWO_PI * u2)             float64, each operation rounded once
    out[j] = O(double(x[j]) + sigma * z(offset + j))       one conversion to O

Everything is vectorised over the element index; the bits and the uniforms are exact, ``log`` and ``cos``
are numpy's (glibc's) float64 functions."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers on ctr[0], ctr[2]
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")       # the float64 nearest 2 pi
Z_MAX = 8.58                             # sqrt(-2 log 2^-53) = 8.5712...
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 of the counters ``ctr`` (four array-likes of 32-bit words, broadcast together) under
    ``key`` (two 32-bit words): four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) for w in ctr])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # a 32 x 32 bit product fits 64 bits
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def bits(seed, stream_id, round_id, i):
    """The four words of the elements ``i`` (an array of indices in [0, 2^64))."""
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed)
    assert 0 <= seed < 1 << 64 and 0 <= int(stream_id) < 1 << 32 and 0 <= int(round_id) < 1 << 32
    return philox4x32_10((i & _MASK, i >> _S32, np.uint64(stream_id), np.uint64(round_id)),
                         (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(x):
    """``(u1, u2)`` of the words ``x``: float64, u1 in (0, 1], u2 in [0, 1), both exact."""
    x0, x1, x2, x3 = (np.asarray(v, dtype=np.uint64) for v in x)
    n1 = ((x0 >> np.uint64(5)) << np.uint64(26)) + (x1 >> np.uint64(6)) + np.uint64(1)
    n2 = ((x2 >> np.uint64(5)) << np.uint64(26)) + (x3 >> np.uint64(6))
    return n1.astype(np.float64) * 2.0 ** -53, n2.astype(np.float64) * 2.0 ** -53


def radius(u1):
    """``sqrt(-2 * log(u1))``, each operation rounded once."""
    return np.sqrt(np.float64(-2.0) * np.log(u1))


def deviates(seed, stream_id, round_id, i):
    """``(z, u1)`` of the elements ``i``: the deviates in float64 and the first uniform (the error metric's
    scale is ``max(1, radius(u1))``)."""
    u1, u2 = uniforms(bits(seed, stream_id, round_id, i))
    return radius(u1) * np.cos(np.float64(TWO_PI) * u2), u1


def apply(x, sigma, z, dtype):
    """``O(double(x) + sigma * z)``: the product and the sum rounded once in float64, one conversion to
    ``dtype``. ``x`` None counts as zeros."""
    z = np.asarray(z, dtype=np.float64)
    base = np.zeros(z.shape, dtype=np.float64) if x is None else np.asarray(x).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (base + np.float64(sigma) * z).astype(dtype)


def index_range(offset, P):
    """The stream indices of ``out[0 .. P)`` at ``offset``."""
    return np.uint64(offset) + np.arange(P, dtype=np.uint64)


def statistics(z):
    """``(mean, std, D * sqrt(n))`` of the sample ``z`` against N(0, 1): D is the Kolmogorov-Smirnov
    distance to the normal distribution function."""
    import math
    z = np.sort(np.asarray(z, dtype=np.float64))
    n = z.size
    cdf = np.array([0.5 * math.erfc(-v / math.sqrt(2.0)) for v in z])
    k = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(k / n - cdf)), float(np.max(cdf - (k - 1.0) / n)))
    return float(z.mean()), float(z.std()), d * math.sqrt(n)
