"""Host reference of the weighted quantile and histogram calls (df_wquant.hip, df_whist.hip) in
pure integers: Python ``int``, or uint64 numpy where a point has many draws (every sum stays
below 2^56).  It builds on resample_ref.quantise (the quantised weights) and quantile_ref.keys
(the totalOrder key); nothing here comes from the library.

    q_j  = rint(ldexp(w_j, 32 − e)) for finite w_j > 0, else 0; wmax = f·2^e, f in [0.5, 1)
    T    = Σ q_j; a point with T = 0 is empty and has the scale (0, 0)
    τ    = max(1, ceil(num·T / 2^32)) for a numerator num in [0, 2^32]
    quantile of a dimension = the draw with the smallest key k such that Σ {q_j : key_j <= k} >= τ
    table bin = Σ q_j over the draws histogram_ref counts there
"""
import numpy as np

import histogram_ref as H
import quantile_ref as Q
import resample_ref as R

ONE = 1 << 32
NAN_BITS = 0x7FC00000


def numerators(probs):
    """num = int(rint(float64(p)·2^32))."""
    return [int(np.rint(np.float64(p) * 4294967296.0)) for p in probs]


def scale(w):
    """One point's Float32 weights → (e, T, q): q the list of Python ints of resample_ref.quantise."""
    w = np.asarray(w, dtype=np.float32).ravel()
    q = R.quantise(w)
    T = sum(q)
    if T == 0:
        return 0, 0, q
    with np.errstate(invalid="ignore"):
        part = np.isfinite(w) & (w > 0)
    _, e = np.frexp(np.float64(w[part].max()))
    return int(e), T, q


def scales(w):
    """(M, N) weights → (e (M,), T (M,)) int64 and q (M, N) uint64."""
    w = np.asarray(w, dtype=np.float32)
    e, T, q = zip(*(scale(row) for row in w))
    return np.array(e, np.int64), np.array(T, np.int64), np.array(q, dtype=np.uint64).reshape(w.shape)


def tau(num, T):
    assert 0 <= num <= ONE and 0 < T < 1 << 56
    return max(1, -((-num * T) >> 32))


def quantile_scan(x, q, num):
    """One dimension of one point: draws x (N,) float32, Python-int weights q, numerator → the bits
    (uint32) of the weighted quantile by a sorted scan, NAN_BITS for an empty point."""
    T = sum(q)
    if T == 0:
        return NAN_BITS
    t = tau(num, T)
    k = Q.keys(np.asarray(x, np.float32))
    c = 0
    for j in np.argsort(k, kind="stable"):
        c += q[j]
        if c >= t:
            return int(Q.values(k[j:j + 1]).view(np.uint32)[0])
    raise AssertionError("tau above T")


def quantile_radix(x, q, num):
    """The same quantile as the device finds it: 4 passes over 8-bit digits of the key, most
    significant first, with 256 sums of q per pass; exactly one bin answers in each pass."""
    T = sum(q)
    if T == 0:
        return NAN_BITS
    rem = tau(num, T)
    k = [int(v) for v in Q.keys(np.asarray(x, np.float32))]
    prefix = 0
    for p in range(4):
        shift = 24 - 8 * p
        h = [0] * 256
        for kj, qj in zip(k, q):
            if qj and (p == 0 or (kj ^ prefix) >> (shift + 8) == 0):
                h[(kj >> shift) & 255] += qj
        assert 1 <= rem <= sum(h)
        below, answers = 0, []
        for b in range(256):
            if below < rem <= below + h[b]:
                answers.append((b, below))
            below += h[b]
        assert len(answers) == 1 and h[answers[0][0]] > 0
        prefix |= answers[0][0] << shift
        rem -= answers[0][1]
    return int(Q.values(np.array([prefix], np.uint32)).view(np.uint32)[0])


def quantiles(draws, w, nums):
    """float32 (M, d, P) of draws (M, N, d) under weights (M, N) at the numerators: per point and
    dimension a stable sort of the keys, a uint64 cumulative sum and a search for τ."""
    draws = np.asarray(draws)
    assert draws.dtype == np.float32 and draws.ndim == 3
    M, N, d = draws.shape
    out = np.full((M, d, len(nums)), NAN_BITS, np.uint32)
    _, T, q = scales(w)
    for i in range(M):
        if T[i] == 0:
            continue
        taus = np.array([tau(n, int(T[i])) for n in nums], np.uint64)
        for k in range(d):
            key = Q.keys(draws[i, :, k])
            order = np.argsort(key, kind="stable")
            cum = np.cumsum(q[i][order], dtype=np.uint64)
            at = np.searchsorted(cum, taus, side="left")
            out[i, k] = Q.values(key[order][at]).view(np.uint32)
    return out.view(np.float32)


def blocks(draws, w, edges, keep):
    """(M, T) uint64: the tables ``keep`` (histogram_ref's layout and bin rule) with Σ q_j per bin."""
    draws = np.asarray(draws)
    assert draws.dtype == np.float32 and draws.ndim == 3
    M, N, d = draws.shape
    bins = H.bins_of(edges)
    _, _, q = scales(w)
    idx = np.full((d, M, N), -1, np.int64)
    for k in range(d):
        if edges[k] is None:
            continue
        e = np.asarray(edges[k], np.float32)
        v = draws[:, :, k]
        j = np.searchsorted(e, v, side="right") - 1
        j[v == e[-1]] = bins[k] - 1
        j[(j < 0) | (j >= bins[k])] = -1
        idx[k] = j
    sizes = H.sizes(keep, bins)
    out = np.zeros((M, sum(sizes)), np.uint64)
    at = 0
    for K, size in zip(keep, sizes):
        ia = idx[K[0]]
        ok = ia >= 0
        at_bin = ia
        if len(K) == 2:
            ib = idx[K[1]]
            ok = ok & (ib >= 0)
            at_bin = ia + int(bins[K[0]]) * ib
        # np.bincount sums float64: the 16-bit halves of q stay exact (below 2^16 · 2^24 each)
        where = (np.arange(M)[:, None] * size + at_bin)[ok]
        lo = np.bincount(where, weights=(q[ok] & np.uint64(0xFFFF)).astype(np.float64), minlength=M * size)
        hi = np.bincount(where, weights=(q[ok] >> np.uint64(16)).astype(np.float64), minlength=M * size)
        flat = (hi.astype(np.uint64) << np.uint64(16)) + lo.astype(np.uint64)
        out[:, at:at + size] = flat.reshape(M, size)
        at += size
    return out


def blocks_brute(draws, w, edges, keep):
    """blocks() by the loop over points, draws and tables in Python ints."""
    draws = np.asarray(draws)
    M, N, _ = draws.shape
    bins = H.bins_of(edges)
    sizes = H.sizes(keep, bins)
    out = [[0] * sum(sizes) for _ in range(M)]
    for i in range(M):
        _, _, q = scale(w[i])
        for j in range(N):
            at = 0
            for K, size in zip(keep, sizes):
                ia = H.bin_of(draws[i, j, K[0]], edges[K[0]])
                ib = H.bin_of(draws[i, j, K[1]], edges[K[1]]) if len(K) == 2 else 0
                if ia >= 0 and ib >= 0:
                    out[i][at + ia + int(bins[K[0]]) * ib] += q[j]
                at += size
    return np.array(out, dtype=np.uint64).reshape(M, sum(sizes))


HOSTILE = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, -1.0, -1e-30, 1e-45, 1e-40, 1.17549435e-38,
                    3.4028235e38, 1.0, 0.5, 3.0, 1e-12], np.float32)


def weight_patterns(M, N, rng):
    """{name: (M, N) float32 weights}: the patterns every weighted call is run against."""
    out = {
        "lognormal3": np.exp(3.0 * rng.standard_normal((M, N))).astype(np.float32),
        "lognormal30": np.exp(np.clip(30.0 * rng.standard_normal((M, N)), -87.0, 87.0)).astype(np.float32),
        "unit": np.ones((M, N), np.float32),
    }
    hot = np.zeros((M, N), np.float32)
    hot[np.arange(M), rng.integers(0, N, M)] = rng.uniform(0.1, 10.0, M).astype(np.float32)
    out["onehot"] = hot
    hostile = rng.uniform(0.0, 2.0, (M, N)).astype(np.float32)
    for i in range(M):
        rows = rng.permutation(N)[:max(N // 2, 1)]
        hostile[i, rows] = rng.choice(HOSTILE, rows.size)
    if M > 1:
        hostile[M // 2] = rng.choice(HOSTILE[:8], N)        # an empty point among others: nothing takes part
    out["hostile"] = hostile
    return out


def plant_draws(x, rng):
    """Into every point and dimension of x (M, N, d), in place: ties, ±0, ±inf and NaN of both signs."""
    M, N, d = x.shape
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0, 1.0, -2.5], np.float32)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)
    special = np.concatenate([special, nan])
    for i in range(M):
        for k in range(d):
            rows = rng.permutation(N)[:max(N // 3, 1)]
            x[i, rows, k] = rng.choice(special, rows.size)
    return x
