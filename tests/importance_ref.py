"""Host reference of the importance-weight calls (df_iw.hip): the stabilised weights in float64,
the exact sums of a point's own Float32 weights, the exact weighted masked sums and weighted
shifted sums with the error bound of an fp64 sum in any order, and the moments from a block."""
import math

import numpy as np

import point_stats_ref as P

U = 2.0 ** -52
FLT_MIN = float(np.finfo(np.float32).tiny)

# The largest distance of the device's expf(logw − m) from float64 np.exp of the same Float32
# difference, in Float32 ulps of the exact value, over the normal results of
# tests/test_gpu_importance.py::test_weights (logw spread over [−100, 0]); measured on an MI355X
# (DESIGN §7).  The test asserts at twice this, rounded up to a whole ulp, and never below
# FLT_MIN in absolute terms (a subnormal result may be flushed).
EXPF_MEASURED_ULP = 0.8374
EXPF_BOUND_ULP = float(math.ceil(2.0 * EXPF_MEASURED_ULP))


def block_entries(d):
    """2 + 2d + d(d+1)/2: the doubles of one point's block [W1, W2 | c | S1w | S2w, a >= b]."""
    return 2 + P.entries(d)


def _fsum(col):
    col = np.asarray(col, np.float64)
    with np.errstate(invalid="ignore"):
        return math.fsum(col) if np.all(np.isfinite(col)) else float(np.sum(col))


def log_max(logw):
    """m (M,) float32: the largest non-NaN logw of every point (NaN for a point of NaN alone)."""
    lw = np.asarray(logw)
    assert lw.dtype == np.float32 and lw.ndim == 2
    return np.fmax.reduce(lw, axis=1)


def weights64(logw):
    """(m (M,) float32, w (M, N) float64): np.exp in float64 of the Float32 difference logw − m."""
    lw = np.asarray(logw)
    m = log_max(lw)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (lw - m[:, None]).astype(np.float32)          # one Float32 subtraction
        return m, np.exp(diff.astype(np.float64))


def ulp32(v):
    """The Float32 spacing at |v| (v float64), as float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def weight_sums(w):
    """(stats (M, 3), bound (M, 2)) of Float32 weights (M, N): W1 = Σ w, W2 = Σ w² and
    #{w > 0}, the sums exact (every term is an exact double: math.fsum), and the accumulation
    bound N · 2^-52 · Σ|term| of W1 and W2."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.ndim == 2
    M, N = w.shape
    w64 = w.astype(np.float64)
    stats, bound = np.zeros((M, 3)), np.zeros((M, 2))
    for i in range(M):
        stats[i] = [_fsum(w64[i]), _fsum(w64[i] * w64[i]), float(np.sum(w[i] > 0))]
        with np.errstate(invalid="ignore"):
            bound[i] = [N * U * np.sum(np.abs(w64[i])), N * U * np.sum(w64[i] * w64[i])]
    return stats, bound


def evidence(m, w1, w2, n_draws):
    """(log Ẑ, stderr of log Ẑ, ESS) from a point's m, W1, W2."""
    N = float(n_draws)
    m, w1, w2 = (np.asarray(v, np.float64) for v in (m, w1, w2))
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (N * w2 / (w1 * w1) - 1.0) / (N - 1.0)
        return m + np.log(w1 / N), np.sqrt(np.where(var < 0.0, 0.0, var)), w1 * w1 / w2


def weighted_ranks(x, draws, w):
    """(wrank (d, M), bound (d, M)): Σ_j w_ij · [draws[i, j, k] < x[k, i]] summed exactly, of
    float32 x (d, M), draws (M, N, d) and weights (M, N), and the bound N · 2^-52 · Σ_j w_ij of
    the accumulation.  IEEE comparison: a tie and a NaN on either side count nothing."""
    x, q, w = np.asarray(x), np.asarray(draws), np.asarray(w)
    assert x.dtype == q.dtype == w.dtype == np.float32
    M, N, d = q.shape
    out, bound = np.zeros((d, M)), np.zeros((d, M))
    for i in range(M):
        w64 = w[i].astype(np.float64)
        with np.errstate(invalid="ignore"):
            for k in range(d):
                out[k, i] = _fsum(w64[q[i, :, k] < x[k, i]])
            bound[:, i] = N * U * np.sum(np.abs(w64))
    return out, bound


def weighted_exact_sums(draws, w):
    """(block, bound), both (M, 2 + 2d + d(d+1)/2): the block df_draw_weighted_stats documents —
    W1, W2, c = draw 0 as a double, S1w = Σ_j w_j (v_j − c), S2w[a, b] = Σ_j w_j (v_ja − c_a)(v_jb
    − c_b) — of float32 draws (M, N, d) and weights (M, N), every term formed in fp64 (the
    conversions, the subtraction, w·(v_a − c_a), then the product) and summed exactly, and the
    bound a device sum must keep to per entry: (N + 2) · 2^-52 · Σ|term|, the bound of
    point_stats_ref.exact_sums with one more rounding per term, for w·(v_a − c_a).  W1 and W2:
    exact terms, N · 2^-52 · Σ|term|.  c is exact: its bound is 0."""
    q, w = np.asarray(draws), np.asarray(w)
    assert q.dtype == np.float32 and w.dtype == np.float32
    M, N, d = q.shape
    a, b = P.pairs(d)
    block = np.zeros((M, block_entries(d)))
    bound = np.zeros_like(block)
    ws, wb = weight_sums(w)
    block[:, :2], bound[:, :2] = ws[:, :2], wb
    for i in range(M):
        c = q[i, 0].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            v = q[i].astype(np.float64) - c              # (N, d)
            wv = w[i].astype(np.float64)[:, None] * v    # one fp64 multiply
            terms = np.concatenate([wv, wv[:, a] * v[:, b]], axis=1)      # (N, d + P)
            block[i, 2:2 + d] = c
            block[i, 2 + d:] = [_fsum(col) for col in terms.T]
            bound[i, 2 + d:] = (N + 2) * U * np.sum(np.abs(terms), axis=0)
    return block, bound


def weighted_moments(block, d, ddof=1):
    """mean (d, M), cov (d, d, M) from blocks (M, 2 + 2d + d(d+1)/2): δ = S1w/W1, mean = c + δ,
    cov = (S2w/W1 − δδᵀ), divided by 1 − W2/W1² unless ddof = 0 — the textbook form, in fp64."""
    blk = np.asarray(block, np.float64).reshape(-1, block_entries(d))
    w1, w2 = blk[:, 0], blk[:, 1]
    c, s1 = blk[:, 2:2 + d], blk[:, 2 + d:2 + 2 * d]
    a, b = P.pairs(d)
    s2 = np.empty((blk.shape[0], d, d))
    s2[:, a, b] = blk[:, 2 + 2 * d:]
    s2[:, b, a] = blk[:, 2 + 2 * d:]
    delta = s1 / w1[:, None]
    cov = s2 / w1[:, None, None] - delta[:, :, None] * delta[:, None, :]
    if ddof:
        cov = cov / (1.0 - w2 / (w1 * w1))[:, None, None]
    return (c + delta).T, np.moveaxis(cov, 0, -1)


def repeated_moments(draws, counts, ddof=0):
    """mean (d, M), cov (d, d, M): the plain two-pass moments of draws (M, N, d) with draw j of
    point i repeated counts[i, j] times, the covariance over the count of rows less ddof.  Integer
    weights are frequencies: the weighted moments at ddof = 0 are these at ddof = 0 (the
    reliability correction 1 − W2/W1² is not the frequency correction 1 − 1/Σn)."""
    q = np.asarray(draws, np.float64)
    means, covs = [], []
    for i in range(q.shape[0]):
        rep = np.repeat(q[i], np.asarray(counts[i], int), axis=0)
        mu = rep.mean(axis=0)
        r = rep - mu
        means.append(mu)
        covs.append(r.T @ r / (rep.shape[0] - ddof))
    return np.stack(means).T, np.moveaxis(np.stack(covs), 0, -1)
