"""Host reference of df_flow_point_stats (df_pstats.hip): exact Float32 comparison counts per
dimension, the exact shifted sums with the error bound of an fp64 sum in any order, mean and
covariance from a block, and the brackets and bounds a device result must meet given fp64
oracle draws."""
import math

import numpy as np

import hpd_ref as H

# the shape of the oracle parity test (tests/test_gpu_point_stats.py) and of its CPU pre-check
ORACLE_M, ORACLE_N = 17, 260
UNDECIDED_CAP = 0.002          # Σ(hi − lo) / (d · M · N), a condition of the issue, not a measurement
U = 2.0 ** -52


def entries(d):
    """S = 2d + d(d+1)/2: the doubles of one point's block [c | S1 | S2, a >= b]."""
    return 2 * d + d * (d + 1) // 2


def pairs(d):
    """(a, b) of S2's entries in block order, index a(a+1)/2 + b with a >= b."""
    return np.tril_indices(d)


def ranks(x, draws):
    """rank[k, i] = #{j : draws[i, j, k] < x[k, i]} of float32 x (d, M) and draws (M, N, d), as
    int32 (d, M).  IEEE comparison: a tie and a NaN on either side count nothing."""
    x = np.asarray(x)
    q = np.asarray(draws)
    assert x.dtype == np.float32 and q.dtype == np.float32 and q.shape[0] == x.shape[1] and q.shape[2] == x.shape[0]
    with np.errstate(invalid="ignore"):
        return np.sum(q < x.T[:, None, :], axis=1).T.astype(np.int32)


def exact_sums(draws):
    """(block, bound), both (M, S): the block df_flow_point_stats documents — c = draw 0 as a
    double, S1 = Σ_j (v_j − c), S2[a, b] = Σ_j (v_ja − c_a)(v_jb − c_b) — of float32 draws
    (M, N, d), with every term formed in fp64 (conversion, then subtraction, then the product)
    and summed exactly (math.fsum), and the bound a device sum must keep to per entry:
    (N + 1) · 2^-52 · Σ|term|.

    An N-term fp64 sum in any order is within (N − 1)·u·Σ|term| (u = 2^-53) to first order; the
    terms themselves differ from the host's by one rounding of the product (the host rounds
    it, a fused multiply-add does not): u·|term| each.  N·u·Σ|term| covers both, and the bound
    is twice that with one more term's worth for the higher orders: (N + 1)·2u·Σ|term|.  c is
    exact: a float converted to double; its bound is 0."""
    q = np.asarray(draws)
    assert q.dtype == np.float32
    M, N, d = q.shape
    a, b = pairs(d)
    block = np.zeros((M, entries(d)))
    bound = np.zeros_like(block)
    for i in range(M):
        c = q[i, 0].astype(np.float64)
        v = q[i].astype(np.float64) - c              # (N, d)
        terms = np.concatenate([v, v[:, a] * v[:, b]], axis=1)      # (N, d + P)
        block[i, :d] = c
        with np.errstate(invalid="ignore"):
            block[i, d:] = [math.fsum(col) if np.all(np.isfinite(col)) else np.sum(col) for col in terms.T]
            bound[i, d:] = (N + 1) * U * np.sum(np.abs(terms), axis=0)
    return block, bound


def moments(block, d, n_draws):
    """mean (d, M) and cov (d, d, M) from blocks (M, S): mean = c + S1/N,
    cov = (S2 − S1 S1ᵀ/N)/(N − 1), in fp64."""
    blk = np.asarray(block, np.float64).reshape(-1, entries(d))
    N = float(n_draws)
    c, s1 = blk[:, :d], blk[:, d:2 * d]
    a, b = pairs(d)
    s2 = np.empty((blk.shape[0], d, d))
    s2[:, a, b] = blk[:, 2 * d:]
    s2[:, b, a] = blk[:, 2 * d:]
    cov = (s2 - s1[:, :, None] * s1[:, None, :] / N) / (N - 1.0)
    return (c + s1 / N).T, np.moveaxis(cov, 0, -1)


def plain_moments(draws64):
    """mean (d, M) and cov (d, d, M) of fp64 draws (M, N, d), the plain two-pass way."""
    q = np.asarray(draws64, np.float64)
    mean = q.mean(axis=1)                                  # (M, d)
    r = q - mean[:, None, :]
    cov = np.einsum("mja,mjb->abm", r, r) / (q.shape[1] - 1)
    return mean.T, cov


def oracle_draws(spec, th, z64, n_draws, tmin, tmax):
    """The fp64 oracle's draws (M, n_draws, d): the base draw z64 (d, M · n_draws) sent forward
    under raw θ (n, M) repeated per point."""
    from oracle import flow_oracle as O

    thn = O.normalize_input(th, tmin, tmax) if th.shape[0] else th
    x64, _ = O.forward(spec, z64, np.repeat(thn, n_draws, axis=1), np.float64)
    return x64.T.reshape(th.shape[1], n_draws, z64.shape[0])


def rank_bracket(x, draws64):
    """(lo, hi), both (d, M): the ranks' bounds from fp64 oracle draws (M, N, d) when every
    Float32 draw is within close's tolerance of its fp64 value: a draw is certainly below the
    point's coordinate if x64 < x − tol(x64), possibly below if x64 < x + tol(x64)."""
    q = np.asarray(draws64, np.float64)
    t = H.close_tol(q)
    xk = np.asarray(x, np.float64).T[:, None, :]
    return np.sum(q < xk - t, axis=1).T, np.sum(q < xk + t, axis=1).T


def moment_bounds(draws64):
    """(mean bound (d, M), cov bound (d, d, M)) for Float32 draws v_j = u_j + δ_j around the
    fp64 oracle's u_j (M, N, d), |δ_jk| <= ε_k = max_j tol(u_jk).

    mean: v̄ − ū = δ̄, |δ̄_k| <= ε_k.
    cov:  v − v̄ = (u − ū) + (δ − δ̄), so (N − 1)·(cov_v − cov_u)_ab
            = Σ (u_a − ū_a)(δ_b − δ̄_b) + Σ (δ_a − δ̄_a)(u_b − ū_b) + Σ (δ_a − δ̄_a)(δ_b − δ̄_b).
          Σ (u_a − ū_a) = 0, so the first sum is Σ (u_a − ū_a) δ_b, at most N·ε_b·mean|u_a − ū_a|;
          the second likewise; the third is at most sqrt(Σ δ_a² Σ δ_b²) <= N·ε_a·ε_b
          (Cauchy-Schwarz; centring lowers a sum of squares).  With m_k = mean_j |u_jk − ū_k| + ε_k
          (the ε on top covers the spread taken about the device's mean instead of the oracle's):
          |cov_v − cov_u|_ab <= N/(N − 1) · (ε_a·m_b + ε_b·m_a + ε_a·ε_b)."""
    q = np.asarray(draws64, np.float64)
    N = q.shape[1]
    eps = np.max(H.close_tol(q), axis=1)                               # (M, d)
    m = np.mean(np.abs(q - q.mean(axis=1, keepdims=True)), axis=1) + eps
    cb = N / (N - 1.0) * (eps[:, :, None] * m[:, None, :] + eps[:, None, :] * m[:, :, None]
                          + eps[:, :, None] * eps[:, None, :])
    return eps.T, np.moveaxis(cb, 0, -1)


def norm_affine(spec):
    """(A, b), each (d,): the lone NormalizationLayer's x = A·z + b per dimension, in fp64."""
    L = spec["layers"][0]
    xmin, xmax = np.asarray(L["x_min"], np.float64), np.asarray(L["x_max"], np.float64)
    al, be = float(L["alpha"]), float(L["beta"])
    return (xmax - xmin) / (be - al), (be * xmin - al * xmax) / (be - al)


def norm_spec(d):
    """A chain of one NormalizationLayer at dimension d, n = 0: no weights, any d."""
    rng = np.random.default_rng(d)
    lo = rng.uniform(-3.0, -0.5, d).astype(np.float32)
    hi = (lo + rng.uniform(0.5, 4.0, d)).astype(np.float32)
    return {"kind": "chain", "layers": [{"kind": "norm", "x_min": lo, "x_max": hi, "alpha": 0.0, "beta": 1.0}]}


def norm61_spec():
    """d = 61: the largest odd d class, d no multiple of 4, 1891 pairs."""
    return norm_spec(61)


def sbc_histogram(ranks_, n_draws, bins):
    """Counts (d, bins) of ranks (d, ...) in ``bins`` equal groups of 0 .. n_draws, by a plain loop."""
    r = np.asarray(ranks_).reshape(np.asarray(ranks_).shape[0], -1)
    width = (n_draws + 1) // bins
    out = np.zeros((r.shape[0], bins), np.int64)
    for k in range(r.shape[0]):
        for v in r[k]:
            out[k, int(v) // width] += 1
    return out
