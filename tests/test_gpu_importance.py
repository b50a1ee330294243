"""GPU tests of the importance-weight calls (df_iw.hip): df_importance_weights,
df_draw_weighted_stats and their Python mirror posterior_draws / importance_weights /
weighted_stats / importance_posterior_stats.

Synthetic numpy draws and log-weights unless a flow is named.  Shapes (M points, N draws, d):
N in {4, 12, 64, 68, 256, 260, 1028} — packed (16 and 5 points per wave), packed full, a wave with
a partial second tile, the wave limit, a workgroup with a partial last trip in which wave 0 has
one trip more, 17 trips; d in {1, 5, 7, 17, 61} — lane groups at E <= 32 (d = 1: 32 groups, d = 5:
3), the shifted-double path without groups (d = 7), the plain path above d = 16, 30 passes of the
lanes over the entries (d = 61); M in {1, 5, 9, 33} — the last wave and the last workgroup partly
filled.  Every N at d = 5, every d at N in {12, 260}, every M at (N, d) = (12, 5) and (260, 5).

Every test after test_weights takes the device's own w_out as its weights.  Flows are untrained:
ESS and log Ẑ are printed, not asserted.  Flow batches (at most 5 · 1028 samples) stay below the
small-kernel crossover, so the bitwise comparisons stay inside one chain-pass kernel family.
"""

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import flows
from densityflows_amd.data import MetaData
from densityflows_amd.hip import run_draw_weighted_stats, run_importance_weights
from helpers import spec_to_element
import importance_ref as I
import point_stats_ref as P
from test_gpu_moments import _bounds, _chain
from test_gpu_score import _spec
from test_gpu_train import _dev, _inputs

pytestmark = pytest.mark.gpu

GUARD = 8
TAIL = 64                       # NaN floats behind every input: they must reach no result

NS = (4, 12, 64, 68, 256, 260, 1028)
DS = (1, 5, 7, 17, 61)
MS = (1, 5, 9, 33)
CASES = sorted({(5, N, 5) for N in NS} | {(5, N, d) for N in (12, 260) for d in DS} |
               {(M, N, 5) for M in MS for N in (12, 260)})
MN_CASES = sorted({(M, N) for M, N, _ in CASES})


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _input(a, cuda):
    """A float32 array as a flat device tensor followed by TAIL NaN floats → the tensor's head
    (of an empty array: the tail, so that an empty call still passes a non-null pointer)."""
    import torch

    flat = np.ascontiguousarray(a, np.float32).ravel()
    buf = torch.full((flat.size + TAIL,), np.nan, dtype=torch.float32, device=cuda)
    buf[:flat.size] = torch.from_numpy(flat).to(cuda)
    return buf[:flat.size] if flat.size else buf


def _weights(cuda, logw, want_w=True, want_stats=True, at=None):
    """One df_importance_weights call on numpy logw (M, N) → (w (M, N) float32, stats (M, 4)
    float64), None for what was not asked for.  Both outputs are followed by GUARD elements (NaN)
    that must survive.  ``at``: the call covers point ``at`` alone, with the pointers advanced."""
    import torch

    M, N = logw.shape
    lw = _input(logw, cuda)
    w = torch.full((M * N + GUARD,), np.nan, dtype=torch.float32, device=cuda) if want_w else None
    st = torch.full((4 * M + GUARD,), np.nan, dtype=torch.float64, device=cuda) if want_stats else None
    if at is None:
        run_importance_weights(lw, M, N, w, st)
    else:
        run_importance_weights(lw[at * N:], 1, N, w[at * N:] if want_w else None, st[4 * at:] if want_stats else None)
    torch.cuda.synchronize()
    nan_bits = _bits(np.float32(np.nan).reshape(1))[0]
    out = [None, None]
    if want_w:
        v = w.cpu().numpy()
        assert np.all(_bits(v[M * N:]) == nan_bits), "w_out written past n_points · n_draws"
        out[0] = v[:M * N].reshape(M, N).copy()
    if want_stats:
        v = st.cpu().numpy()
        assert np.all(np.isnan(v[4 * M:])), "stats_out written past 4 · n_points"
        out[1] = v[:4 * M].reshape(M, 4).copy()
    return tuple(out)


def _wstats(cuda, q, w, x, want_rank=True, want_sums=True, at=None):
    """One df_draw_weighted_stats call on numpy draws (M, N, d), weights (M, N), points (d, M) →
    (wrank (d, M), blocks (M, S)) float64, None for what was not asked for; guards as above."""
    import torch

    M, N, d = q.shape
    S = I.block_entries(d)
    xs, wb = _input(q, cuda), _input(w, cuda)
    xb = _input(np.ascontiguousarray(x.T), cuda) if want_rank else None
    rk = torch.full((d * M + GUARD,), np.nan, dtype=torch.float64, device=cuda) if want_rank else None
    sb = torch.full((S * M + GUARD,), np.nan, dtype=torch.float64, device=cuda) if want_sums else None
    if at is None:
        run_draw_weighted_stats(xs, wb, xb, d, M, N, rk, sb)
    else:
        run_draw_weighted_stats(xs[at * N * d:], wb[at * N:], xb[at * d:] if want_rank else None, d, 1, N,
                                rk[at * d:] if want_rank else None, sb[at * S:] if want_sums else None)
    torch.cuda.synchronize()
    out = [None, None]
    if want_rank:
        v = rk.cpu().numpy()
        assert np.all(np.isnan(v[d * M:])), "wrank_out written past d · n_points"
        out[0] = v[:d * M].reshape(M, d).T.copy()
    if want_sums:
        v = sb.cpu().numpy()
        assert np.all(np.isnan(v[S * M:])), "sums_out written past n_points blocks"
        out[1] = v[:S * M].reshape(M, S).copy()
    return tuple(out)


def _logw(M, N):
    """Log-weights spread over [−100, 0] below a per-point offset: exp(logw − max) reaches the
    subnormal range (below exp(−87.3))."""
    rng = np.random.default_rng(1000 * M + N)
    return (rng.uniform(-100.0, 0.0, (M, N)) + rng.uniform(-50.0, 50.0, (M, 1))).astype(np.float32)


_CASE = {}


def _case(cuda, M, N, d):
    """(q (M, N, d), x (d, M), w (M, N) — the device's own — and the exact references), computed
    once per shape and shared, never modified."""
    key = (M, N, d)
    if key not in _CASE:
        rng = np.random.default_rng(7 * M + 11 * N + 13 * d)
        q = (rng.standard_normal((M, N, d)) * rng.uniform(0.5, 3.0, d) + rng.uniform(-5.0, 100.0, d)).astype(np.float32)
        x = (q.mean(axis=1).T + rng.standard_normal((d, M)) * 0.5).astype(np.float32)
        x[0, 0] = q[0, 1, 0]                                   # a tie: it counts nothing
        w, _ = _weights(cuda, _logw(M, N), want_stats=False)
        block, bound = I.weighted_exact_sums(q, w)
        rank, rbound = I.weighted_ranks(x, q, w)
        _CASE[key] = (q, x, w, block, bound, rank, rbound)
    return _CASE[key]


# ---------------------------------------------------------------------------
# 1. the weights
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", MN_CASES)
def test_weights(cuda, M, N):
    """m is np.max exactly; w_out against float64 np.exp of the same Float32 difference, within
    importance_ref.EXPF_BOUND_ULP Float32 ulps of the exact value or FLT_MIN.  Measured on an
    MI355X over these inputs: see importance_ref.EXPF_MEASURED_ULP."""
    lw = _logw(M, N)
    w, st = _weights(cuda, lw)
    m, ref = I.weights64(lw)
    np.testing.assert_array_equal(_bits64(st[:, 0]), _bits64(m.astype(np.float64)))
    np.testing.assert_array_equal(m, np.max(lw, axis=1))
    assert np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(w.max(axis=1) == 1.0)
    err = np.abs(w.astype(np.float64) - ref)
    ulp = I.ulp32(ref)
    normal = ref >= I.FLT_MIN
    worst = float(np.max(err[normal] / ulp[normal]))
    sub = float(np.max(err[~normal])) if np.any(~normal) else 0.0
    flushed = int(np.sum((w == 0) & ~normal))
    print(f"M={M} N={N}: expf distance {worst:.4f} ulp over {int(normal.sum())} normal results; "
          f"{int((~normal).sum())} subnormal results, {flushed} returned as 0, worst absolute {sub:.3e}")
    assert np.all(err <= np.maximum(I.EXPF_BOUND_ULP * ulp, I.FLT_MIN)), worst
    # either output alone: the same bytes
    w2, _ = _weights(cuda, lw, want_stats=False)
    _, st2 = _weights(cuda, lw, want_w=False)
    np.testing.assert_array_equal(_bits(w2), _bits(w))
    np.testing.assert_array_equal(_bits64(st2), _bits64(st))


# ---------------------------------------------------------------------------
# 2. the sums of the first call, exact against its own weights
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", MN_CASES)
def test_weight_sums_exact_against_own_weights(cuda, M, N):
    w, st = _weights(cuda, _logw(M, N))
    ref, bound = I.weight_sums(w)
    err = np.abs(st[:, 1:3] - ref[:, :2])
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    lz, se, ess = I.evidence(st[:, 0], st[:, 1], st[:, 2], N)
    print(f"M={M} N={N}: W1, W2 error / bound {worst:.3f}; n_pos {st[:3, 3]}, ESS {ess[:3]}, log Z {lz[:3]}")
    assert np.all(err <= bound), worst
    np.testing.assert_array_equal(st[:, 3], ref[:, 2])
    assert np.all(st[:, 3] >= 1) and np.all(st[:, 3] <= N)


# ---------------------------------------------------------------------------
# 3. the weighted sums, exact against their own inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,d", CASES)
def test_weighted_sums_exact_against_own_inputs(cuda, M, N, d):
    q, x, w, ref, bound, rref, rbound = _case(cuda, M, N, d)
    rk, blk = _wstats(cuda, q, w, x)
    assert np.all(np.isfinite(rk)) and np.all(np.isfinite(blk)), "outputs not fully overwritten"
    np.testing.assert_array_equal(_bits64(blk[:, 2:2 + d]), _bits64(q[:, 0, :].astype(np.float64)))   # c = draw 0
    err = np.abs(blk - ref)
    tiny = np.finfo(np.float64).tiny
    worst = float(np.max(np.delete(err / np.maximum(bound, tiny), np.s_[2:2 + d], axis=1)))
    rerr = np.abs(rk - rref)
    rworst = float(np.max(rerr / np.maximum(rbound, tiny)))
    print(f"M={M} N={N} d={d}: sums error / bound {worst:.3f}, wrank error / bound {rworst:.3f}; "
          f"cdf {(rk / blk[:, 0])[:, 0][:4]}")
    assert np.all(err <= bound), worst
    assert np.all(rerr <= rbound), rworst
    # the other template instances return the same bits
    r2, _ = _wstats(cuda, q, w, x, want_sums=False)
    _, b3 = _wstats(cuda, q, w, x, want_rank=False)
    np.testing.assert_array_equal(_bits64(r2), _bits64(rk))
    np.testing.assert_array_equal(_bits64(b3), _bits64(blk))


# ---------------------------------------------------------------------------
# 4. unit weights are the unweighted call
# ---------------------------------------------------------------------------

def _norm_chain(d):
    spec = P.norm_spec(d)
    return spec, d, 0, spec_to_element(spec).hip()


@pytest.mark.parametrize("name", ["readme", "norm61", "norm7", "norm16"])
@pytest.mark.parametrize("N", [12, 68, 260, 1028])
def test_unit_weights_are_point_stats(cuda, name, N):
    import torch

    spec, d, n, h = _norm_chain(int(name[4:])) if name.startswith("norm") else _chain(name)
    M = 5
    x, th = _inputs(d, n, M)
    S = P.entries(d)
    rank = torch.empty(d * M, dtype=torch.int32, device=cuda)
    sums = torch.empty(S * M, dtype=torch.float64, device=cuda)
    draws = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    xb = _dev(x, cuda)
    h.run_point_stats(xb, _dev(th, cuda) if n else None, M, N, 0, 31, 2, rank, sums, draws)
    # constant log-weights per point: unit weights, log Ẑ = the constant, ESS = N, all exact
    consts = np.array([-3.25, 0.0, 17.5, -88.0, 1e-3], np.float32)
    lw = np.repeat(consts[:, None], N, axis=1)
    iw = dfa.importance_weights(torch.from_numpy(lw).to(cuda))
    assert isinstance(iw.w, torch.Tensor) and iw.w.shape == (M, N)
    np.testing.assert_array_equal(_bits(iw.w.cpu().numpy()), _bits(np.ones((M, N), np.float32)))
    np.testing.assert_array_equal(iw.log_evidence, consts.astype(np.float64))
    np.testing.assert_array_equal(iw.ess, np.full(M, float(N)))
    np.testing.assert_array_equal(iw.efficiency, np.ones(M))
    np.testing.assert_array_equal(iw.n_positive, np.full(M, N))
    np.testing.assert_array_equal(iw.log_evidence_stderr, np.zeros(M))
    SW = I.block_entries(d)
    wrank = torch.full((d * M,), np.nan, dtype=torch.float64, device=cuda)
    wsums = torch.full((SW * M,), np.nan, dtype=torch.float64, device=cuda)
    run_draw_weighted_stats(draws, iw.w.reshape(-1), xb, d, M, N, wrank, wsums)
    torch.cuda.synchronize()
    blk = wsums.cpu().numpy().reshape(M, SW)
    np.testing.assert_array_equal(_bits64(blk[:, 2:]), _bits64(sums.cpu().numpy().reshape(M, S)))
    np.testing.assert_array_equal(blk[:, :2], np.full((M, 2), float(N)))
    np.testing.assert_array_equal(wrank.cpu().numpy(), rank.cpu().numpy().astype(np.float64))
    # the Python mirror: posterior_stats' moments bit for bit
    st = dfa.weighted_stats(draws.view(M, N, d), iw, x)
    pm, pc = flows.moments_from_sums(sums.cpu().numpy(), d, N)
    np.testing.assert_array_equal(_bits64(st.mean), _bits64(pm))
    np.testing.assert_array_equal(_bits64(st.cov), _bits64(pc))
    np.testing.assert_array_equal(st.cdf, rank.cpu().numpy().reshape(M, d).T / float(N))
    np.testing.assert_array_equal(st.ess, np.full(M, float(N)))


# ---------------------------------------------------------------------------
# 5. reproducible and independent
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,d", [(5, 12, 5), (5, 68, 5), (5, 260, 5), (5, 12, 61), (5, 260, 61)])
def test_reproducible_and_independent(cuda, M, N, d):
    """Two calls give the same bytes; point i computed alone, with the pointers advanced, gives
    the bytes of its block in the batch call.  The guards behind every output and the NaN region
    behind every input are checked in the helpers: the results here are finite."""
    q, x, w, *_ = _case(cuda, M, N, d)
    lw = _logw(M, N)
    w1, s1 = _weights(cuda, lw)
    w2, s2 = _weights(cuda, lw)
    np.testing.assert_array_equal(_bits(w1), _bits(w2))
    np.testing.assert_array_equal(_bits64(s1), _bits64(s2))
    np.testing.assert_array_equal(_bits(w1), _bits(w))
    rk, blk = _wstats(cuda, q, w, x)
    rk2, blk2 = _wstats(cuda, q, w, x)
    np.testing.assert_array_equal(_bits64(rk), _bits64(rk2))
    np.testing.assert_array_equal(_bits64(blk), _bits64(blk2))
    assert np.all(np.isfinite(w1)) and np.all(np.isfinite(s1)) and np.all(np.isfinite(rk)) and np.all(np.isfinite(blk))
    for i in (1, M - 1):
        wi, si = _weights(cuda, lw, at=i)
        np.testing.assert_array_equal(_bits(wi[i]), _bits(w1[i]))
        np.testing.assert_array_equal(_bits64(si[i]), _bits64(s1[i]))
        assert np.all(np.isnan(np.delete(wi, i, axis=0))) and np.all(np.isnan(np.delete(si, i, axis=0)))
        ri, bi = _wstats(cuda, q, w, x, at=i)
        np.testing.assert_array_equal(_bits64(ri[:, i]), _bits64(rk[:, i]))
        np.testing.assert_array_equal(_bits64(bi[i]), _bits64(blk[i]))
        assert np.all(np.isnan(np.delete(ri, i, axis=1))) and np.all(np.isnan(np.delete(bi, i, axis=0)))


def test_empty_call_writes_nothing(cuda):
    w, st = _weights(cuda, np.zeros((0, 8), np.float32))          # the guards (every element) are checked inside
    assert w.shape == (0, 8) and st.shape == (0, 4)
    rk, blk = _wstats(cuda, np.zeros((0, 8, 5), np.float32), np.zeros((0, 8), np.float32), np.zeros((5, 0), np.float32))
    assert rk.shape == (5, 0) and blk.shape == (0, I.block_entries(5))
    iw = dfa.importance_weights(np.zeros((0, 8), np.float32))
    assert iw.w.shape == (0, 8) and iw.ess.shape == (0,)
    st = dfa.weighted_stats(np.zeros((0, 8, 5), np.float32), iw)
    assert st.mean.shape == (5, 0) and st.cov.shape == (5, 5, 0) and st.cdf is None


# ---------------------------------------------------------------------------
# 6. non-finite inputs stay in their point
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", [12, 68, 260])
def test_nonfinite_logw_stays_in_its_point(cuda, N):
    M = 5
    lw = _logw(M, N)
    w, st = _weights(cuda, lw)
    bad = lw.copy()
    j_nan = int(np.argmin(lw[1]))                 # not the largest: m_1 stays
    bad[1, j_nan] = np.nan
    bad[2, 5] = np.inf
    bad[3, :] = -np.inf
    wb, sb = _weights(cuda, bad)
    for i in (0, 4):                              # the clean points, bit for bit
        np.testing.assert_array_equal(_bits(wb[i]), _bits(w[i]))
        np.testing.assert_array_equal(_bits64(sb[i]), _bits64(st[i]))
    # a NaN logw: that weight and W1, W2 of its point; m and n_pos stay numbers
    assert np.isnan(wb[1, j_nan]) and np.sum(np.isnan(wb[1])) == 1
    np.testing.assert_array_equal(_bits(np.delete(wb[1], j_nan)), _bits(np.delete(w[1], j_nan)))
    assert sb[1, 0] == st[1, 0] and np.isnan(sb[1, 1]) and np.isnan(sb[1, 2])
    assert sb[1, 3] == np.sum(np.delete(w[1], j_nan) > 0)
    # +inf: m = +inf, that weight NaN, every other weight 0, NaN sums
    assert sb[2, 0] == np.inf and np.isnan(wb[2, 5]) and np.all(np.delete(wb[2], 5) == 0)
    assert np.isnan(sb[2, 1]) and np.isnan(sb[2, 2]) and sb[2, 3] == 0
    # −inf alone: m = −inf, every weight NaN, NaN sums
    assert sb[3, 0] == -np.inf and np.all(np.isnan(wb[3])) and np.isnan(sb[3, 1]) and np.isnan(sb[3, 2])
    assert sb[3, 3] == 0
    # −inf beside finite values: weight 0, counted out of n_pos, sums finite
    some = lw.copy()
    low = np.argsort(lw[0])[:3]                   # not the largest: m_0 stays
    some[0, low] = -np.inf
    ws, ss = _weights(cuda, some)
    assert np.all(ws[0, low] == 0) and np.all(np.isfinite(ss[0])) and ss[0, 0] == st[0, 0]
    np.testing.assert_array_equal(_bits(np.delete(ws[0], low)), _bits(np.delete(w[0], low)))
    assert ss[0, 3] == np.sum(np.delete(w[0], low) > 0)
    np.testing.assert_array_equal(_bits64(ss[1:]), _bits64(st[1:]))


@pytest.mark.parametrize("N,d", [(12, 5), (68, 5), (260, 5), (260, 17)])
def test_nan_draw_stays_in_its_entries(cuda, N, d):
    M = 5
    q, x, w, *_ = _case(cuda, M, N, d)
    rk, blk = _wstats(cuda, q, w, x)
    bad = q.copy()
    k1 = min(1, d - 1)
    bad[1, 2, k1] = np.nan                        # a later draw: S1w[k1] and every S2w[k1, .]
    bad[3, 0, 0] = np.nan                         # draw 0: the shift of dimension 0 as well
    rb, bb = _wstats(cuda, bad, w, x)
    for i in (0, 2, 4):
        np.testing.assert_array_equal(_bits64(bb[i]), _bits64(blk[i]))
        np.testing.assert_array_equal(_bits64(rb[:, i]), _bits64(rk[:, i]))
    a, b = P.pairs(d)
    for i, k, shift in ((1, k1, False), (3, 0, True)):
        expect = np.zeros(I.block_entries(d), bool)
        expect[2 + k] = shift
        expect[2 + d + k] = True
        expect[2 + 2 * d:] = (a == k) | (b == k)
        np.testing.assert_array_equal(np.isnan(bb[i]), expect)
        np.testing.assert_array_equal(_bits64(bb[i][~expect]), _bits64(blk[i][~expect]))
        # a NaN counts nothing: the weighted rank of that dimension is the exact masked sum still
        ref, bound = I.weighted_ranks(x[:, i:i + 1], bad[i:i + 1], w[i:i + 1])
        assert np.all(np.abs(rb[:, i] - ref[:, 0]) <= bound[:, 0])
        others = np.arange(d) != k
        np.testing.assert_array_equal(_bits64(rb[others, i]), _bits64(rk[others, i]))


# ---------------------------------------------------------------------------
# 7. the pipeline on a flow
# ---------------------------------------------------------------------------

def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


@pytest.mark.parametrize("name,M,N", [("readme", 8, 64), ("cfg5", 2, 12)])
def test_pipeline_on_a_flow(cuda, name, M, N):
    import torch

    flow = _flow(name)
    d, n = flow.d, flow.n
    seed, offset = 515, 4
    x, th = _inputs(d, n, M)
    q, lq = dfa.posterior_draws(flow, th, n_draws=N, seed=seed, offset=offset)
    assert q.shape == (M, N, d) and lq.shape == (M, N) and q.dtype == lq.dtype == np.float32
    # log q is df_flow_hpd_ranks' draws_logpdf_out at the same (seed, offset), bit for bit
    h = flow.hip()
    rank = torch.empty(M, dtype=torch.int32, device=cuda)
    dl = torch.full((M * N,), np.nan, dtype=torch.float32, device=cuda)
    h.run_hpd_ranks(_dev(x, cuda), _dev(th, cuda), M, N, 0, seed, offset, rank, None, dl)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(lq.ravel()), _bits(dl.cpu().numpy()))
    only = dfa.posterior_draws(flow, th, n_draws=N, seed=seed, offset=offset, return_logpdf=False)
    np.testing.assert_array_equal(_bits(only), _bits(q))

    centre = torch.linspace(-0.5, 0.5, d, device=cuda)
    calls = []

    def log_target(draws, theta):                # an unnormalised Gaussian around `centre`
        calls.append(tuple(draws.shape))
        assert isinstance(draws, torch.Tensor) and draws.device.type == "cuda"
        return -0.5 * ((draws - centre) ** 2).sum(dim=-1)

    st, iw = dfa.importance_posterior_stats(flow, th, log_target, n_draws=N, x=x, seed=seed, offset=offset)
    assert calls == [(M, N, d)]
    # the composition of the three pieces, bit for bit
    qt, lqt = dfa.posterior_draws(flow, th, n_draws=N, seed=seed, offset=offset, as_tensor=True)
    assert isinstance(qt, torch.Tensor) and qt.device.type == "cuda"
    np.testing.assert_array_equal(_bits(qt.cpu().numpy()), _bits(q))
    iw2 = dfa.importance_weights(log_target(qt, th), lqt)
    st2 = dfa.weighted_stats(qt, iw2, x)
    np.testing.assert_array_equal(_bits(iw.w.cpu().numpy()), _bits(iw2.w.cpu().numpy()))
    for a_, b_ in ((iw.log_evidence, iw2.log_evidence), (iw.ess, iw2.ess), (iw.log_evidence_stderr, iw2.log_evidence_stderr),
                   (st.mean, st2.mean), (st.cov, st2.cov), (st.cdf, st2.cdf), (st.ess, st2.ess)):
        np.testing.assert_array_equal(_bits64(a_), _bits64(b_))
    np.testing.assert_array_equal(iw.n_positive, iw2.n_positive)
    # numpy in, numpy out: the same numbers through the host
    iw3 = dfa.importance_weights(log_target(qt, th).cpu().numpy(), lq)
    assert isinstance(iw3.w, np.ndarray)
    np.testing.assert_array_equal(_bits(iw3.w), _bits(iw.w.cpu().numpy()))
    st3 = dfa.weighted_stats(q, iw3.w, x)
    np.testing.assert_array_equal(_bits64(st3.cov), _bits64(st.cov))
    np.testing.assert_array_equal(st.ess, iw.ess)
    assert st.mean.shape == (d, M) and st.cov.shape == (d, d, M) and st.cdf.shape == (d, M)
    nz = iw.normalized()
    assert nz.dtype == torch.float64 and nz.shape == (M, N)
    print(f"{name} (untrained): ESS {iw.ess}, efficiency {iw.efficiency}, log Z {iw.log_evidence} "
          f"± {iw.log_evidence_stderr}, n_pos {iw.n_positive}")
