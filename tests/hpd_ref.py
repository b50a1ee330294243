"""Host reference of the HPD rank (expected-coverage) test: exact Float32 comparison counts,
the bracket a rank must lie in given fp64 oracle densities, and the coverage curve restated."""
import numpy as np

# the shape of the oracle parity test (tests/test_gpu_hpd.py) and of its CPU pre-check
ORACLE_M, ORACLE_N = 17, 260


def ranks(lp_points, lp_draws):
    """rank_i = #{k : lp_draws[i, k] > lp_points[i]} of float32 values (M,) and (M, N), as
    int32.  IEEE comparison: a NaN on either side counts nothing."""
    p = np.asarray(lp_points)
    q = np.asarray(lp_draws)
    assert p.dtype == np.float32 and q.dtype == np.float32 and q.shape[0] == p.shape[0]
    with np.errstate(invalid="ignore"):
        return np.sum(q > p[:, None], axis=1).astype(np.int32)


def close_tol(ref, rtol=1e-5, atol_scale=1e-5):
    """tol(v) = atol + rtol·|v| of helpers.close for the expected array ``ref``."""
    ref = np.asarray(ref, np.float64)
    atol = atol_scale * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)
    return atol + rtol * np.abs(ref)


def bracket(lp64_points, lp64_draws):
    """(lo, hi): the ranks' bounds from fp64 densities of the points (M,) and their draws
    (M, N) when every Float32 density is within close's tolerance of its fp64 value.  A draw is
    certainly above its point if lp64_ik − lp64_i > tol(lp64_ik) + tol(lp64_i), possibly above
    if the difference is > −(the same)."""
    p = np.asarray(lp64_points, np.float64)
    q = np.asarray(lp64_draws, np.float64)
    t = close_tol(q) + close_tol(p)[:, None]
    diff = q - p[:, None]
    return np.sum(diff > t, axis=1), np.sum(diff > -t, axis=1)


def oracle_lp(spec, x, th, z64, n_draws, tmin, tmax):
    """fp64 oracle densities of the points x (d, M) under raw θ (n, M) → (M,), and of the
    draws: the base draw z64 (d, M · n_draws) sent forward under θ repeated per point →
    (M, n_draws), lp = logpdf(MvNormal, z) − ldj."""
    from oracle import flow_oracle as O

    thn = O.normalize_input(th, tmin, tmax) if th.shape[0] else th
    lp_p = O.flow_logpdf(spec, np.asarray(x, np.float64), thn, np.float64)
    _, ldj = O.forward(spec, z64, np.repeat(thn, n_draws, axis=1), np.float64)
    return lp_p, (O.mvnormal_logpdf(z64, np.float64) - ldj).reshape(x.shape[1], n_draws)


def expected_coverage(levels, credibility=None):
    """(c, share of levels <= c) for every credibility c (default linspace(0, 1, 101)), the
    plain way: one comparison of every level with every c."""
    lv = np.asarray(levels, np.float64).ravel()
    c = np.linspace(0.0, 1.0, 101) if credibility is None else np.asarray(credibility, np.float64).ravel()
    return c, np.array([np.count_nonzero(lv <= v) / lv.size for v in c])
