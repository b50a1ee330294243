"""GPU tests of the order-statistics calls (df_quant.hip): df_order_statistics,
df_flow_point_quantiles and their Python mirrors order_statistics / posterior_quantiles /
credible_intervals.

An order statistic of Float32 draws is one of the draws: every comparison with the host
reference (tests/quantile_ref.py: a sort of the totalOrder keys) is bit for bit.

Chains and kernel families: those of tests/test_gpu_point_stats.py; every batch here (at most
2 · 4100 = 8200 samples) lies below the README-class chain's small-kernel crossover, so every
bitwise comparison of draws stays inside one chain-pass family.

The selection kernel has one form (radix select) and one cutoff in N: a wave per point up to
N = 256, a workgroup per point above; (3, 256), (3, 260) and (2, 256), (2, 260) stand on it.
What a launch holds in LDS at once depends on the number of orders Q: at Q = 32 a workgroup
takes 2 dimensions and a wave 1 at a time, at Q = 6 they take 10 and 2, so every d > 2 below is
walked in groups in one mapping or both.

No test states a statistical claim: the models are untrained.  The intervals of one point are
printed.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from helpers import close
import point_stats_ref as P
import quantile_ref as Q
from test_gpu_moments import _bounds, _chain
from test_gpu_point_stats import GUARD, INT32_MIN, _any_chain, _bits, _bits64, _flow, _stats
from test_gpu_train import _dev, _inputs

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def _select(cuda, q, orders):
    """One df_order_statistics call on numpy draws (M, N, d) → (M, d, Q) float32.  The output is
    followed by GUARD NaNs that must survive, and every element must have been written."""
    import torch

    M, N, d = q.shape
    nq = len(orders)
    xs = torch.from_numpy(np.ascontiguousarray(q)).to(cuda)
    out = torch.full((M * d * nq + GUARD,), np.nan, dtype=torch.float32, device=cuda)
    out.view(torch.int32)[:M * d * nq] = 0x7FC12345          # a NaN no test data holds
    dfa.hip.run_order_statistics(xs, d, M, N, orders, out)
    torch.cuda.synchronize()
    v = out.cpu().numpy()
    assert np.all(_bits(v[M * d * nq:]) == NAN_BITS), "out written past d · n_points · n_orders"
    assert np.all(_bits(v[:M * d * nq]) != 0x7FC12345), "out not fully written"
    return v[:M * d * nq].reshape(M, d, nq).copy()


def _quant(h, cuda, x, th, N, orders, chunk=0, seed=77, offset=3, quant=True, ranks=True, sums=True, draws=True,
           shift=0, M=None):
    """One df_flow_point_quantiles call, as _stats of tests/test_gpu_point_stats.py →
    (quantiles (M, d, Q) float32, ranks (d, M), blocks (M, S), draws (M, N, d)), None for what was
    not asked for; every output is followed by GUARD elements that must survive."""
    import torch

    d = x.shape[0]
    M = x.shape[1] if M is None else M
    n = th.shape[0]
    S = P.entries(d)
    nq = len(orders) if orders is not None else 0
    qbuf = torch.full((M * d * nq + GUARD,), np.nan, dtype=torch.float32, device=cuda) if quant else None
    rank = torch.full((d * M + GUARD,), INT32_MIN, dtype=torch.int32, device=cuda) if ranks else None
    sbuf = torch.full((S * M + GUARD,), np.nan, dtype=torch.float64, device=cuda) if sums else None
    dbuf = torch.full((4 + d * M * N + GUARD,), np.nan, dtype=torch.float32, device=cuda) if draws else None
    xb = (_dev(x, cuda) if M else torch.zeros(d, dtype=torch.float32, device=cuda)) if ranks else None
    h.run_point_quantiles(xb, _dev(th, cuda) if n and M else None, M, N, chunk, seed, offset, orders, qbuf, rank,
                          sbuf, dbuf[shift:] if draws else None)
    torch.cuda.synchronize()
    out = [None, None, None, None]
    if quant:
        v = qbuf.cpu().numpy()
        assert np.all(_bits(v[M * d * nq:]) == NAN_BITS), "quant_out written past d · n_points · n_orders"
        out[0] = v[:M * d * nq].reshape(M, d, nq).copy()
    if ranks:
        r = rank.cpu().numpy()
        assert np.all(r[d * M:] == INT32_MIN), "rank_out written past d · n_points"
        assert np.all(r[:d * M] != INT32_MIN), "rank_out not fully written"
        out[1] = r[:d * M].reshape(M, d).T.copy()
    if sums:
        v = sbuf.cpu().numpy()
        assert np.all(np.isnan(v[S * M:])), "sums_out written past n_points blocks"
        out[2] = v[:S * M].reshape(M, S).copy()
    if draws:
        v = dbuf.cpu().numpy()
        assert np.all(_bits(v[:shift]) == NAN_BITS) and np.all(_bits(v[shift + d * M * N:]) == NAN_BITS), \
            "draws_out written outside d · n_points · n_draws"
        out[3] = v[shift:shift + d * M * N].reshape(M, N, d).copy()
    return tuple(out)


def _order_sets(N):
    """[0]; [N − 1]; the two middle orders; six unsorted orders with one repeat; 32 orders."""
    six = [N - 1, N // 2, 0, (N // 4) % N, N // 2, (3 * N // 4) % N]
    many = [int(v) for v in np.random.default_rng(N).integers(0, N, 30)] + [0, N - 1]
    return [[0], [N - 1], [N // 2 - 1, N // 2], six, many]


# ---------------------------------------------------------------------------
# 1. df_order_statistics against the sort of the keys, bit for bit
# ---------------------------------------------------------------------------

# The mapping edges of the per-point kernels (tests/test_gpu_point_stats.py) — N = 4 and 12 (most
# lanes of a wave past the point's last vector), 64, 68, the last N of the wave mapping (256) and
# the first of the workgroup mapping (260: the fifth vector row of d = 1 is one lane of wave 1),
# 4100 (every thread several vectors), 257 points past one workgroup of 4 — and, with M = 2, the
# cutoff 256 and the cutoff + 4 once more.
SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 256), (3, 260), (257, 4), (2, 4100), (2, 256), (2, 260)]
DIMS = [1, 5, 8, 32, 61]


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_order_statistics_exact(cuda, d, M, N):
    rng = np.random.default_rng(1000 * d + N + M)
    q = rng.standard_normal((M, N, d)).astype(np.float32)
    q[0, :, d - 1] = q[0, 0, d - 1]                                    # the last dimension of point 0: one value
    q[M - 1, rng.integers(0, N, max(N // 3, 1)), 0] = np.float32(0.5)  # duplicates in the first of the last point
    for orders in _order_sets(N):
        got = _select(cuda, q, orders)
        np.testing.assert_array_equal(_bits(got), _bits(Q.order_stats(q, orders)), err_msg=f"orders {orders}")
    # a second call gives the same bytes
    orders = _order_sets(N)[3]
    np.testing.assert_array_equal(_bits(_select(cuda, q, orders)), _bits(_select(cuda, q, orders)))


# Many draws per point: every thread of the workgroup walks many vectors, a bin's count and the
# residual rank pass 2^8 and 2^16, and (second case) half of the draws share one value, so that one
# bin holds 2^19 of them in every pass.
@pytest.mark.parametrize("d,M,N", [(3, 2, 65540), (1, 1, 1 << 20)])
def test_order_statistics_many_draws(cuda, d, M, N):
    rng = np.random.default_rng(N)
    q = rng.standard_normal((M, N, d)).astype(np.float32)
    if d == 1:
        q[0, rng.permutation(N)[:N // 2], 0] = np.float32(-0.125)
    for orders in ([0, N - 1], [N // 2 - 1, N // 2, 65535, 65536, N // 4, N // 4],
                   [int(v) for v in rng.integers(0, N, 32)]):
        np.testing.assert_array_equal(_bits(_select(cuda, q, orders)), _bits(Q.order_stats(q, orders)),
                                      err_msg=f"orders {orders}")


def _two_values(N, s, rng):
    col = np.where(np.arange(N) < s, np.float32(-1.25), np.float32(2.5)).astype(np.float32)
    return rng.permutation(col)


def _from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def _patterns(N, r, rng):
    """name → column of N float32 in which order r falls inside the pattern."""
    u = lambda lo, hi, size=N: rng.integers(lo, hi, size, dtype=np.int64).astype(np.uint32)
    sign = lambda: (u(0, 2) << np.uint32(31))
    normal = rng.standard_normal(N).astype(np.float32)
    nan_mix = normal.copy()
    k = max(N // 4, 1)
    nan_mix[:k] = _from_bits(np.uint32(0x7F800001) + u(0, 0x7FFFFF, k))           # +NaN, any payload
    nan_mix[k:2 * k] = _from_bits(np.uint32(0xFF800001) + u(0, 0x7FFFFF, k))      # −NaN
    inf_mix = normal.copy()
    inf_mix[:k] = np.inf
    inf_mix[k:2 * k] = -np.inf
    return {
        "normal": normal,
        "one value": np.full(N, 1.5, np.float32),
        "two values, split at the order": _two_values(N, r, rng),
        "two values, split below the order": _two_values(N, max(r - 1, 0), rng),
        "two values, split above the order": _two_values(N, min(r + 1, N), rng),
        "equal top 24 bits": _from_bits(np.uint32(0x3FC0AB00) | u(0, 256)),
        "equal top 24 bits, negative": _from_bits(np.uint32(0xBFC0AB00) | u(0, 256)),
        "signed zeros": _from_bits(sign()),
        "infinities": rng.permutation(inf_mix),
        "NaNs of both signs": rng.permutation(nan_mix),
        "only NaNs": _from_bits((np.uint32(0x7F800001) + u(0, 0x7FFFFF)) | sign()),
        "denormals": _from_bits(u(1, 0x800000) | sign()),
        "ascending": np.arange(N, dtype=np.float32) - np.float32(N // 2),
        "descending": np.float32(N // 2) - np.arange(N, dtype=np.float32),
    }


# N = 12 and 68: a wave per point (one and two trips of its lanes over d = 5); 260 and 1028: a
# workgroup per point (the hand-over between the four waves' counts)
@pytest.mark.parametrize("N", [12, 68, 260, 1028])
def test_order_statistics_patterns(cuda, N):
    """Dimension 2 of d = 5 carries the pattern while its neighbours vary (the stride of the
    (d, N) layout); point 1 carries it in every dimension."""
    rng = np.random.default_rng(N)
    d, r = 5, N // 2 - 1
    orders = sorted({0, max(r - 1, 0), r, r + 1, N - 1}) + [r]
    pats = _patterns(N, r, rng)
    for name, col in pats.items():
        assert col.dtype == np.float32 and col.shape == (N,)
        q = rng.standard_normal((3, N, d)).astype(np.float32)
        q[0, :, 2] = col
        q[1] = col[:, None]
        q[2, :, 2] = col[::-1]
        got = _select(cuda, q, orders)
        ref = Q.order_stats(q, orders)
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=name)
        np.testing.assert_array_equal(_bits(got[0, 2]), _bits(got[2, 2]), err_msg=name)     # the same multiset
    print(f"N={N}: {len(pats)} patterns at orders {orders}")


# ---------------------------------------------------------------------------
# 2. the flow's own draws
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", [(3, 12), (5, 68), (2, 516)])
@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "cfg5", "norm61"])
def test_exact_against_own_draws(cuda, name, M, N):
    spec, d, n, h = _any_chain(name)
    x, th = _inputs(d, n, M)
    orders = [N - 1, N // 2, 0, N // 4, N // 2, N // 2 - 1]                 # unsorted, one repeat
    qt, r, blk, q = _quant(h, cuda, x, th, N, orders)
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(qt)), "outputs not fully overwritten"
    np.testing.assert_array_equal(_bits(qt), _bits(Q.order_stats(q, orders)))
    # the other three outputs are df_flow_point_stats' at the same (seed, offset)
    r0, b0, q0 = _stats(h, cuda, x, th, N)
    np.testing.assert_array_equal(_bits(q), _bits(q0))
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(_bits64(blk), _bits64(b0))
    # the quantiles alone
    q1, _, _, _ = _quant(h, cuda, x, th, N, orders, ranks=False, sums=False, draws=False)
    np.testing.assert_array_equal(_bits(q1), _bits(qt))
    # without the quantiles: the orders are not looked at
    _, r2, b2, _ = _quant(h, cuda, x, th, N, None, quant=False, draws=False)
    np.testing.assert_array_equal(r2, r0)
    np.testing.assert_array_equal(_bits64(b2), _bits64(b0))
    # a draws buffer off the 16-byte boundary: the same values everywhere
    q5, r5, b5, d5 = _quant(h, cuda, x, th, N, orders, shift=1)
    np.testing.assert_array_equal(_bits(q5), _bits(qt))
    np.testing.assert_array_equal(r5, r)
    np.testing.assert_array_equal(_bits64(b5), _bits64(blk))
    np.testing.assert_array_equal(_bits(d5), _bits(q))


# ---------------------------------------------------------------------------
# 3. independence of chunking and of the other points
# ---------------------------------------------------------------------------

# M = 7, N = 260: chunk 0 and 2^14 take the 1820 draws at once, 520 two points at a time (the
# last chunk one point), 260 and 100 (below N) one point at a time.  All below the small-kernel
# crossover.
@pytest.mark.parametrize("name", ["readme", "cfg2"])
def test_chunking_and_other_points(cuda, name):
    spec, d, n, h = _chain(name)
    M, N, seed, offset = 7, 260, 11, 4
    x, th = _inputs(d, n, M)
    orders = [41, 42, 129, 130, 217, 218]
    qt, r, blk, q = _quant(h, cuda, x, th, N, orders, seed=seed, offset=offset)
    np.testing.assert_array_equal(_bits(qt), _bits(Q.order_stats(q, orders)))
    for chunk in (260, 520, 100, 1 << 14, 0):
        qc, rc, bc, dc = _quant(h, cuda, x, th, N, orders, chunk=chunk, seed=seed, offset=offset)
        np.testing.assert_array_equal(_bits(qc), _bits(qt), err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(rc, r, err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits64(bc), _bits64(blk), err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits(dc), _bits(q))
    # point 3 alone, at its own counter
    q3, r3, b3, d3 = _quant(h, cuda, x[:, 3:4], th[:, 3:4], N, orders, seed=seed, offset=offset + d * 3 * N // 4)
    np.testing.assert_array_equal(_bits(q3[0]), _bits(qt[3]))
    np.testing.assert_array_equal(r3[:, 0], r[:, 3])
    np.testing.assert_array_equal(_bits64(b3[0]), _bits64(blk[3]))
    np.testing.assert_array_equal(_bits(d3[0]), _bits(q[3]))


# ---------------------------------------------------------------------------
# 4. parity with the fp64 oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "cfg5"])
def test_against_oracle(cuda, name):
    """Order statistics are 1-Lipschitz in the sup norm: |device − oracle order statistic| <=
    max_j |draw_j − oracle draw_j| over the point's dimension, the right side from the same call's
    draws_out.  The draws themselves are held by helpers.close."""
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = P.ORACLE_M, P.ORACLE_N, 2025, 1
    x, th = _inputs(d, n, M)
    orders = sorted({0, N - 1} | {int(v) for p in (0.025, 0.16, 0.5, 0.84, 0.975) for v in Q.linear_orders(p, N)[:2]})
    qt, _, _, q = _quant(h, cuda, x, th, N, orders, seed=seed, offset=offset, ranks=False, sums=False)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M * N, d).T.astype(np.float64)
    q64 = P.oracle_draws(spec, th, z64, N, *_bounds(n))                  # (M, N, d)
    ok, rq = close(q, q64)
    assert ok, rq
    ref = np.sort(q64, axis=1)[:, orders, :].transpose(0, 2, 1)          # (M, d, Q)
    bound = np.max(np.abs(q.astype(np.float64) - q64), axis=1)           # (M, d)
    err = np.abs(qt.astype(np.float64) - ref)
    print(f"{name}: draws parity {rq:.3f}; worst order-statistic error {err.max():.3e} under bound "
          f"{bound.max():.3e}; orders {orders}")
    assert np.all(err <= bound[:, :, None])


# ---------------------------------------------------------------------------
# 5. d = 61: the closed form of a lone NormalizationLayer
# ---------------------------------------------------------------------------

def test_norm61_closed_form(cuda):
    """x = A·z + b is monotone per dimension: the device's order statistic is that affine map of
    the order statistic of the base draw (order r, or N − 1 − r where A < 0), within the draws'
    parity tolerance."""
    import torch

    spec, d, n, h = _any_chain("norm61")
    M, N, seed, offset = 5, 260, 99, 2
    x, th = _inputs(d, n, M)
    orders = [0, 41, 42, 129, 130, 217, 218, N - 1]
    qt, _, _, q = _quant(h, cuda, x, th, N, orders, seed=seed, offset=offset, ranks=False, sums=False)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M, N, d).astype(np.float64)
    A, b = P.norm_affine(spec)
    zs = np.sort(z64, axis=1)
    o = np.asarray(orders)
    pick = np.where(A[None, None, :] < 0, zs[:, N - 1 - o, :], zs[:, o, :])          # (M, Q, d)
    ref = (A * pick + b).transpose(0, 2, 1)                                           # (M, d, Q)
    ok, ratio = close(qt, ref)
    print(f"norm61: order statistics against A·z_(r) + b: parity ratio {ratio:.3f}")
    assert ok, ratio
    np.testing.assert_array_equal(_bits(qt), _bits(Q.order_stats(q, orders)))


# ---------------------------------------------------------------------------
# 6. Python
# ---------------------------------------------------------------------------

def test_posterior_quantiles(cuda):
    import torch

    flow = _flow("readme")
    d, n, dims, N, seed = 5, 1, (2, 5, 7), 64, 19
    M = 70
    x, th = _inputs(d, n, M)
    xa = np.asfortranarray(x).reshape((d,) + dims, order="F")
    tha = np.asfortranarray(th).reshape((n,) + dims, order="F")
    probs = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)
    qv, st, draws = dfa.posterior_quantiles(flow, tha, probs=probs, n_draws=N, x=xa, seed=seed, return_stats=True,
                                            return_draws=True)
    assert qv.shape == (len(probs), d) + dims and qv.dtype == np.float64
    assert draws.shape == (M, N, d) and draws.dtype == np.float32
    ref = np.quantile(draws.astype(np.float64), probs, axis=1)                  # (P, M, d)
    _, bnd = Q.quantiles(draws, probs)                                          # (P, d, M)
    got = qv.reshape(len(probs), d, M, order="F")
    assert np.all(np.abs(got - ref.transpose(0, 2, 1)) <= bnd)
    # the PointStats are posterior_stats' at the same seed
    s0 = dfa.posterior_stats(flow, tha, n_draws=N, x=xa, seed=seed)
    assert isinstance(st, dfa.PointStats) and st.n_draws == N
    np.testing.assert_array_equal(st.ranks, s0.ranks)
    np.testing.assert_array_equal(_bits64(st.mean), _bits64(s0.mean))
    np.testing.assert_array_equal(_bits64(st.cov), _bits64(s0.cov))
    # the quantiles alone; device tensors in, chunked; an NTuple θ
    q1 = dfa.posterior_quantiles(flow, tha, probs=probs, n_draws=N, seed=seed)
    np.testing.assert_array_equal(_bits64(q1), _bits64(qv))
    tht = torch.from_numpy(np.ascontiguousarray(tha)).to(cuda)
    q2 = dfa.posterior_quantiles(flow, tht, probs=probs, n_draws=N, seed=seed, chunk=128)
    np.testing.assert_array_equal(_bits64(q2), _bits64(qv))
    a = dfa.posterior_quantiles(flow, (1.25,), n_draws=N, dims=dims, seed=seed)
    b = dfa.posterior_quantiles(flow, np.full((n,) + dims, 1.25, np.float32), n_draws=N, seed=seed)
    assert a.shape == (3, d) + dims
    np.testing.assert_array_equal(_bits64(a), _bits64(b))
    # credible intervals: rows of posterior_quantiles
    lo, med, hi = dfa.credible_intervals(flow, tha, level=0.68, n_draws=N, seed=seed)
    rows = dfa.posterior_quantiles(flow, tha, probs=((1 - 0.68) / 2, 0.5, (1 + 0.68) / 2), n_draws=N, seed=seed)
    np.testing.assert_array_equal(_bits64(lo), _bits64(rows[0]))
    np.testing.assert_array_equal(_bits64(med), _bits64(rows[1]))
    np.testing.assert_array_equal(_bits64(hi), _bits64(rows[2]))
    np.testing.assert_array_equal(_bits64(med), _bits64(qv[3]))
    assert np.all(lo <= med) and np.all(med <= hi)
    lo95, med95, hi95 = dfa.credible_intervals(flow, tha, level=0.95, n_draws=N, seed=seed)
    assert np.all(lo95 <= lo) and np.all(hi <= hi95)
    np.testing.assert_array_equal(_bits64(med95), _bits64(med))
    j = (0, 0, 0)
    print("readme (untrained), point 0: median [68 % interval] per dimension: " +
          ", ".join(f"{med[(k,) + j]:.3f} [{lo[(k,) + j]:.3f}, {hi[(k,) + j]:.3f}]" for k in range(d)))
    # order_statistics on the returned draws: numpy in, and a device tensor in
    orders = [0, 31, 32, 63, 31]
    os_np = dfa.order_statistics(draws, orders)
    assert isinstance(os_np, np.ndarray) and os_np.shape == (M, d, 5) and os_np.dtype == np.float32
    np.testing.assert_array_equal(_bits(os_np), _bits(Q.order_stats(draws, orders)))
    os_t = dfa.order_statistics(torch.from_numpy(draws).to(cuda), orders)
    assert isinstance(os_t, torch.Tensor) and os_t.is_cuda
    np.testing.assert_array_equal(_bits(os_t.cpu().numpy()), _bits(os_np))


def test_posterior_quantiles_unconditional(cuda):
    flow = _flow("cfg2")
    d = flow.d
    N, M = 128, 40
    qv, draws = dfa.posterior_quantiles(flow, n_draws=N, dims=(M,), seed=5, return_draws=True)
    assert qv.shape == (3, d, M)
    ref = np.quantile(draws.astype(np.float64), (0.16, 0.5, 0.84), axis=1).transpose(0, 2, 1)
    _, bnd = Q.quantiles(draws, (0.16, 0.5, 0.84))
    assert np.all(np.abs(qv - ref) <= bnd)
    x, _ = _inputs(d, 0, M)
    q2, st = dfa.posterior_quantiles(flow, n_draws=N, x=x, seed=5, return_stats=True)
    np.testing.assert_array_equal(_bits64(q2), _bits64(qv))
    s0 = dfa.posterior_stats(flow, n_draws=N, x=x, seed=5)
    np.testing.assert_array_equal(st.ranks, s0.ranks)
    np.testing.assert_array_equal(_bits64(st.cov), _bits64(s0.cov))
    lo, med, hi = dfa.credible_intervals(flow, n_draws=N, dims=(M,), seed=5, level=0.68)
    np.testing.assert_array_equal(_bits64(med), _bits64(qv[1]))
    assert np.all(lo <= med) and np.all(med <= hi)


def test_empty_call_writes_nothing(cuda):
    import torch

    spec, d, n, h = _chain("readme")
    x, th = _inputs(d, n, 0)
    qt, r, blk, q = _quant(h, cuda, x, th, 8, [0, 7], M=0)       # the guards (every element) are checked inside
    assert qt.shape == (0, d, 2) and r.shape == (d, 0) and blk.shape == (0, P.entries(d)) and q.shape == (0, 8, d)
    out = torch.full((GUARD,), np.nan, dtype=torch.float32, device=cuda)
    xs = torch.zeros(16, dtype=torch.float32, device=cuda)
    dfa.hip.run_order_statistics(xs, d, 0, 8, [0, 7], out)
    torch.cuda.synchronize()
    assert np.all(_bits(out.cpu().numpy()) == NAN_BITS)
    flow = _flow("readme")
    e = dfa.posterior_quantiles(flow, np.zeros((n, 0), np.float32), n_draws=8, seed=1)
    assert e.shape == (3, d, 0)
    assert dfa.order_statistics(np.zeros((0, 8, d), np.float32), [0]).shape == (0, d, 1)
