"""GPU tests of sampling with densities and of the moment reductions (df_moments.hip):
df_flow_sample_logpdf, df_flow_sample_logpdf_moments, df_train_score_moments,
df_train_fisher and their Python mirror.

Bounds.  The reduction adds exact fp64 terms (a product of two floats converted to double
has 48 significant bits) in some fixed order, so any order of B terms is within
(B − 1)·2⁻⁵³·Σ|term| of the exact sum; the tests hold every entry to B·2⁻⁵²·Σ_j|term_j|
against math.fsum of the same terms.  Densities are held to helpers.close at its defaults
(the tolerance logpdf parity uses), scores to the project's gradient criterion (G_RTOL,
G_ATOL of tests/test_gpu_train.py), propagated into the sums where sums are compared.

No test states a statistical claim (mean score ≈ 0, F ≈ −Hessian): the device's Philox
draw cannot be reproduced on a CPU to pre-check one; mean_score / stderr is printed.
"""
import math

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from densityflows_amd.train import Adam, HIPTrainer
from helpers import close, spec_to_element
from oracle import flow_oracle as O
import score_ref as R
from test_gpu_score import _run, _spec, _trainer
from test_gpu_train import (G_ATOL, G_RTOL, _dev, _flat_oracle_grads, _gpu_grad, _inputs, _tensor_slices)

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52


def _bounds(n):
    return np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32)


def _chain(name):
    """(spec, d, n, HIPChain with the θ bounds (−1, 3) per row)."""
    spec, d, n = _spec(name)
    h = spec_to_element(spec).hip()
    if n:
        h.set_theta_bounds(*_bounds(n))
    return spec, d, n, h


def _n10_spec(rng):
    """d = 5 under n = 10 conditions, smooth activations: a 10 × 10 score matrix takes the
    reduction through its 8-row tiles (pairs (0,0), (0,1), (1,1), the last rows partial)."""
    kw = dict(hidden=16, bias_scale=0.1, out_scale=0.5)
    return {"kind": "chain", "layers": [
        O.rnvp_layer(rng, O.coupling_axes(5, [1, 3, 5], n=10), act="tanh", **kw),
        O.rnvp_layer(rng, O.coupling_axes(5, [2, 4], n=10), act="softplus", **kw)]}


def _moments_spec(name):
    if name == "n10":
        return _n10_spec(np.random.default_rng(0)), 5, 10
    return _spec(name)


def _host_block(lp, g):
    """The moment block of (lp (B,), g (m, B)) float32 values: exact fp64 terms, math.fsum.
    Returns (block, Σ|term| per entry)."""
    lp = np.asarray(lp, np.float64)
    g = np.zeros((0, lp.shape[0])) if g is None else np.asarray(g, np.float64)
    m = g.shape[0]
    terms = [np.ones_like(lp), lp, lp * lp] + [g[a] for a in range(m)]
    terms += [g[a] * g[b] for b in range(m) for a in range(m)]          # column-major (a fastest)
    block = np.array([math.fsum(t) for t in terms])
    mag = np.array([math.fsum(np.abs(t)) for t in terms])
    return block, mag


def _score_block(tr, x, th, cuda, accumulate=False, out=None):
    import torch

    B = x.shape[1]
    n = th.shape[0]
    if out is None:
        out = torch.full((3 + n + n * n,), np.nan, dtype=torch.float64, device=cuda)
    tr.score_moments(_dev(x, cuda), _dev(th, cuda) if n else None, B, out, accumulate)
    torch.cuda.synchronize()
    return out.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------
# 1. sample with density
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
@pytest.mark.parametrize("B", [1, 17, 1000])
def test_sample_logpdf(cuda, name, B):
    import torch

    spec, d, n, h = _chain(name)
    seed, offset = 1234 + B, 5
    th = np.random.default_rng(2).uniform(-1, 3, (n, B)).astype(np.float32)
    thb = _dev(th, cuda) if n else None
    f32 = lambda k, fill=np.nan: torch.full((k,), fill, dtype=torch.float32, device=cuda)
    # the draw and the library's own forward of it
    z = f32(d * B)
    h.random_normal(z, d * B, seed, offset)
    xf, ldjf = f32(d * B), f32(B)
    h.run("forward", z, thb, xf, ldjf, B, flow=True)
    x, lp = f32(d * B), f32(B)
    h.run_sample_logpdf(x, lp, thb, False, B, seed, offset)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x.cpu().numpy(), xf.cpu().numpy())
    lpn = lp.cpu().numpy()
    assert np.all(np.isfinite(lpn)), "logpdf_out not fully overwritten"
    # the fp64 oracle on that draw, the base term in fp64
    z64 = z.cpu().numpy().reshape(B, d).T.astype(np.float64)
    thn = O.normalize_input(th, *_bounds(n)) if n else th
    xo, ldjo = O.forward(spec, z64, thn, np.float64)
    ok, r = close(lpn, O.mvnormal_logpdf(z64, np.float64) - ldjo)
    assert ok, r
    # lp = base − ldj with the forward pass's own ldj bits, in the documented Float32 order
    zf = z.cpu().numpy().reshape(B, d).T
    s = zf[0] * zf[0]
    for k in range(1, d):
        s = s + zf[k] * zf[k]
    base = -(np.float32(d) * np.float32(O.LOG2PI) + s) / np.float32(2)
    np.testing.assert_array_equal(lpn, base - ldjf.cpu().numpy())
    # a null logpdf_out leaves x as it is
    x2 = f32(d * B)
    h.run_sample_logpdf(x2, None, thb, False, B, seed, offset)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x2.cpu().numpy(), x.cpu().numpy())
    # theta_broadcast 1 against the same θ in every column
    if n:
        one = np.array([0.25, 2.5, -0.5][:n] + [1.0] * max(0, n - 3), np.float32)
        xa, lpa, xb, lpb = f32(d * B), f32(B), f32(d * B), f32(B)
        h.run_sample_logpdf(xa, lpa, _dev(one[:, None], cuda), True, B, seed, offset)
        h.run_sample_logpdf(xb, lpb, _dev(np.repeat(one[:, None], B, axis=1), cuda), False, B, seed, offset)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(xa.cpu().numpy(), xb.cpu().numpy())
        np.testing.assert_array_equal(lpa.cpu().numpy(), lpb.cpu().numpy())
    # for the record: the round trip through the inverse pass, not asserted
    back = f32(B)
    h.run_logpdf(x, thb, back, B)
    torch.cuda.synchronize()
    print(f"{name} B={B}: max |lp - df_flow_logpdf(x)| = {np.max(np.abs(lpn - back.cpu().numpy())):.3e}, "
          f"oracle violation ratio {r:.3f}")


def test_sample_logpdf_empty_batch(cuda):
    _, d, n, h = _chain("readme")
    h.run_sample_logpdf(None, None, None, False, 0, 1, 0)


# ---------------------------------------------------------------------------
# 2. the reduction alone
# ---------------------------------------------------------------------------

# DF_GRID_CUS=2: the reduction's grid is 2 CUs · kMomWgPerCu (2) = 4 workgroups of kMomThreads
# (256) samples per trip, 1024 samples a trip.  1297 = 1024 + 256 + 17 is 6 tiles: two trips
# per workgroup, 3 workgroups, the last one's second trip holds 17 samples.  2321 = 2048 + 256
# + 17 is 10 tiles: three trips per workgroup, 4 workgroups, the last one holds the 17-sample
# tile alone.
@pytest.mark.parametrize("name,B,cus", [(nm, B, None) for nm in ("readme", "pre", "cfg2") for B in (1, 17, 1000)] +
                         [("n10", 1000, None), ("readme", 1297, "2"), ("pre", 2321, "2")])
def test_score_moments_against_host_sum(cuda, monkeypatch, name, B, cus):
    if cus:
        monkeypatch.setenv("DF_GRID_CUS", cus)
    spec, d, n = _moments_spec(name)
    x, th = _inputs(d, n, B)
    tr = _trainer(spec)
    lp, _, gth = _run(tr, x, th, cuda)
    want, mag = _host_block(lp, gth)
    got = _score_block(tr, x, th, cuda)                  # accumulate = 0 over a NaN-filled block
    assert got.shape == (3 + n + n * n,) and np.all(np.isfinite(got))
    assert got[0] == B
    err = np.abs(got - want)
    print(f"{name} B={B}: max err / bound = {np.max(err / np.maximum(B * U52 * mag, 1e-300)):.3g}")
    assert np.all(err <= B * U52 * mag), (err, B * U52 * mag)
    outer = got[3 + n:].reshape(n, n, order="F")
    np.testing.assert_array_equal(_bits(outer), _bits(outer.T))
    # a second call is bitwise the first
    np.testing.assert_array_equal(_bits(_score_block(tr, x, th, cuda)), _bits(got))
    # accumulate = 1: one fp64 add per entry onto what stands there
    import torch

    x2, th2 = _inputs(d, n, 17, seed=2)
    other = _score_block(tr, x2, th2, cuda)
    out = torch.from_numpy(other.copy()).to(cuda)
    acc = _score_block(tr, x, th, cuda, accumulate=True, out=out)
    np.testing.assert_array_equal(_bits(acc), _bits(other + got))


def test_score_moments_empty_batch(cuda):
    import torch

    spec, d, n = _spec("readme")
    tr = _trainer(spec)
    out = torch.full((5,), 7.0, dtype=torch.float64, device=cuda)
    tr.score_moments(None, None, 0, out, True)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 7.0)
    tr.score_moments(None, None, 0, out, False)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0.0)


def test_score_moments_nonfinite_propagates(cuda):
    """A non-finite per-sample value reaches the entries it touches and no other: a NaN x
    gives a NaN lp (both lp sums are NaN), and the score entries are NaN exactly where the
    sweep's own gθ of that sample is."""
    spec, d, n = _spec("readme")
    x, th = _inputs(d, n, 300)
    x[:, 277] = np.nan
    tr = _trainer(spec)
    lp, _, gth = _run(tr, x, th, cuda)
    assert np.isnan(lp[277]) and np.sum(np.isnan(lp)) == 1
    want, mag = _host_block(lp, gth)
    got = _score_block(tr, x, th, cuda)
    assert got[0] == 300 and np.isnan(got[1]) and np.isnan(got[2])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= 300 * U52 * mag[ok])


# ---------------------------------------------------------------------------
# 3. trainer state
# ---------------------------------------------------------------------------

def test_score_moments_leaves_the_step_alone(cuda):
    spec, x, th = _spec("readme")[0], *_inputs(5, 1, 1000)
    tr, twin = _trainer(spec), _trainer(spec)
    g0, lp0 = _gpu_grad(tr, x, th, cuda)
    _score_block(tr, x[:, :333], th[:, :333], cuda)
    np.testing.assert_array_equal(tr.grad().detach().cpu().numpy(), g0)
    tr.apply()
    g1, lp1 = _gpu_grad(twin, x, th, cuda)
    twin.apply()
    np.testing.assert_array_equal(g1, g0)
    assert lp1 == lp0
    np.testing.assert_array_equal(tr.get_params(), twin.get_params())


# ---------------------------------------------------------------------------
# 4. chunking
# ---------------------------------------------------------------------------

def _chunks(n_samples, chunk):
    return [(s, min(chunk, n_samples - s)) for s in range(0, n_samples, chunk)]


def test_fisher_chunks_replay(cuda):
    """df_train_fisher over four chunks (the last partial) is the host's loop of
    df_flow_sample → df_train_score_moments with the blocks added in order, bit for bit —
    also under DF_THETA_GIVEN, which the call neither follows nor changes."""
    import torch

    spec, d, n, h = _chain("pre")
    tr = HIPTrainer(h, Adam())
    one = np.array([0.5, 2.0], np.float32)
    thvec = _dev(one[:, None], cuda)
    N, chunk, seed, offset = 1000, 256, 99, 3
    out = torch.full((3 + n + n * n,), np.nan, dtype=torch.float64, device=cuda)
    tr.fisher(thvec, N, out, chunk, seed, offset)
    torch.cuda.synchronize()
    whole = out.cpu().numpy().copy()
    acc = np.zeros_like(whole)
    for start, ln in _chunks(N, chunk):
        xb = torch.empty(d * ln, dtype=torch.float32, device=cuda)
        h.run_sample(xb, thvec, True, ln, seed, offset + d * start // 4)
        blk = torch.zeros_like(out)
        tr.score_moments(xb, _dev(np.repeat(one[:, None], ln, axis=1), cuda), ln, blk)   # θ raw (AUTO, bounds set)
        torch.cuda.synchronize()
        acc = acc + blk.cpu().numpy()
    assert whole[0] == N
    np.testing.assert_array_equal(_bits(whole), _bits(acc))
    tr.set_theta_input(_lib.DF_THETA_GIVEN)
    tr.fisher(thvec, N, out, chunk, seed, offset)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(whole))
    # the setting stands: θ is still read as given
    x, th = _inputs(d, n, 64)
    given = _score_block(tr, x, th, cuda)
    lp, _, gth = _run(tr, x, th, cuda)
    want, mag = _host_block(lp, gth)
    assert np.all(np.abs(given - want) <= 64 * U52 * mag)
    ref = R.logpdf_grad(spec, x, th)
    assert close(gth, ref[2], G_RTOL, G_ATOL)[0]


@pytest.mark.parametrize("name", ["cfg2", "wide"])
def test_sample_logpdf_moments_chunks_replay(cuda, name):
    import torch

    spec, d, n, h = _chain(name)
    one = np.array([0.25, 2.5, -0.5][:n], np.float32)
    thvec = _dev(one[:, None], cuda) if n else None
    N, chunk, seed, offset = 1000, 256, 31, 2
    out = torch.full((3,), np.nan, dtype=torch.float64, device=cuda)
    h.run_sample_logpdf_moments(thvec, N, chunk, seed, offset, out)
    torch.cuda.synchronize()
    whole = out.cpu().numpy().copy()
    acc = np.zeros(3)
    for start, ln in _chunks(N, chunk):
        off = offset + d * start // 4
        blk = torch.full((3,), np.nan, dtype=torch.float64, device=cuda)
        h.run_sample_logpdf_moments(thvec, ln, chunk, seed, off, blk)      # one chunk: 0 + c_i
        xb = torch.empty(d * ln, dtype=torch.float32, device=cuda)
        lpb = torch.empty(ln, dtype=torch.float32, device=cuda)
        h.run_sample_logpdf(xb, lpb, thvec, True, ln, seed, off)
        torch.cuda.synchronize()
        want, mag = _host_block(lpb.cpu().numpy(), None)
        b = blk.cpu().numpy()
        assert np.all(np.abs(b - want) <= ln * U52 * mag), (b, want)
        acc = acc + b
    assert whole[0] == N
    np.testing.assert_array_equal(_bits(whole), _bits(acc))
    # n_samples = 0: the block is zeroed
    h.run_sample_logpdf_moments(thvec, 0, chunk, seed, offset, out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 0.0)


# ---------------------------------------------------------------------------
# 5. end to end against the oracle
# ---------------------------------------------------------------------------

def test_fisher_against_oracle(cuda):
    import torch

    spec, d, n, h = _chain("pre")
    tr = HIPTrainer(h, Adam())
    one = np.array([0.5, 2.0], np.float32)
    thvec = _dev(one[:, None], cuda)
    N, seed = 1000, 2024
    out = torch.full((3 + n + n * n,), np.nan, dtype=torch.float64, device=cuda)
    tr.fisher(thvec, N, out, 0, seed, 0)
    xb = torch.empty(d * N, dtype=torch.float32, device=cuda)
    h.run_sample(xb, thvec, True, N, seed, 0)
    torch.cuda.synchronize()
    m = dfa.ScoreMoments(out.cpu().numpy(), n)
    x = xb.cpu().numpy().reshape(N, d).T
    lp, _, g, kink = R.logpdf_grad(spec, x, np.repeat(one[:, None], N, axis=1), *_bounds(n))
    assert m.count == N
    # the per-sample score tolerance the project holds, propagated into the means
    eps = G_ATOL * np.max(np.abs(g), axis=1, keepdims=True) + G_RTOL * np.abs(g)
    ag = np.abs(g)
    fsum = lambda t: math.fsum(t) / N
    for a in range(n):
        red = N * U52 * fsum(ag[a])                                   # the reduction's own rounding
        assert abs(m.mean_score[a] - fsum(g[a])) <= fsum(eps[a]) + red
        for b in range(n):
            bound = fsum(ag[a] * eps[b] + ag[b] * eps[a] + eps[a] * eps[b]) + N * U52 * fsum(ag[a] * ag[b])
            err = abs(m.fisher[a, b] - fsum(g[a] * g[b]))
            print(f"F[{a},{b}] = {m.fisher[a, b]:.6g}, |err| / bound = {err / bound:.3g}")
            assert err <= bound
    # the lp sums under close's tolerance, summed the same way
    tol = 1e-5 * max(1.0, float(np.max(np.abs(lp)))) + 1e-5 * np.abs(lp)
    assert abs(m.lp_sum - math.fsum(lp)) <= math.fsum(tol) + N * U52 * math.fsum(np.abs(lp))
    assert abs(m.lp_sqsum - math.fsum(lp * lp)) <= math.fsum((2 * np.abs(lp) + tol) * tol) + N * U52 * math.fsum(lp * lp)
    np.testing.assert_array_equal(_bits(m.outer), _bits(m.outer.T))
    se = np.sqrt(np.maximum(np.diag(m.score_cov), 0) / N)
    print(f"mean_score / stderr = {m.mean_score / se}, entropy = {m.entropy:.5f} ± {m.entropy_stderr:.5f}")


# ---------------------------------------------------------------------------
# 6. class limits
# ---------------------------------------------------------------------------

def test_layerwise_trainer_unsupported_and_usable(cuda):
    import torch

    spec, d, n, h = _chain("wide")
    B = 64
    x, th = _inputs(d, n, B)
    tr = HIPTrainer(h, Adam())
    tr.set_theta_input(_lib.DF_THETA_GIVEN)
    out = torch.zeros(3 + n + n * n, dtype=torch.float64, device=cuda)
    with pytest.raises(_lib.UnsupportedError, match="hidden width > 64"):
        tr.score_moments(_dev(x, cuda), _dev(th, cuda), B, out)
    with pytest.raises(_lib.UnsupportedError, match="hidden width > 64"):
        tr.fisher(_dev(np.ones((n, 1), np.float32), cuda), 64, out)
    g, lpsum = _gpu_grad(tr, x, th, cuda)
    loss, ref = O.nll_and_grad(spec, x, th)
    ref = _flat_oracle_grads(spec, ref)
    assert abs(-lpsum / B - loss) <= 1e-5 * max(1.0, abs(loss))
    for sl in _tensor_slices(spec):
        ok, r = close(g[sl], ref[sl], G_RTOL, G_ATOL)
        assert ok, r


def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


def test_entropy_on_a_wide_chain(cuda):
    flow = _flow("wide")
    th = (0.25, 2.5, -0.5)
    m = dfa.entropy(flow, 1000, th, chunk=512, seed=11)
    assert m.n == 0 and m.count == 1000 and m.fisher.shape == (0, 0)
    assert np.isfinite(m.entropy) and m.entropy_stderr > 0
    # the same draws through sample_logpdf, chunk by chunk
    acc, mags = np.zeros(3), np.zeros(3)
    for start, ln in _chunks(1000, 512):
        _, lp = dfa.sample_logpdf(flow, ln, th, seed=11, offset=8 * start // 4)
        want, mag = _host_block(lp.cpu().numpy(), None)
        acc, mags = acc + want, mags + mag
    got = np.array([m.count, m.lp_sum, m.lp_sqsum])
    assert np.all(np.abs(got - acc) <= 1000 * U52 * mags)
    print(f"wide: H = {m.entropy:.5f} ± {m.entropy_stderr:.5f}")


def test_unconditional_block_has_three_entries(cuda):
    flow = _flow("cfg2")
    m = dfa.fisher_information(flow, (), 256, seed=5)
    assert m.n == 0 and m.count == 256 and m.fisher.shape == (0, 0) and m.mean_score.shape == (0,)
    assert np.isfinite(m.entropy)
    x = dfa.sample(flow, 256, seed=5)
    m2 = dfa.score_moments(flow, x)
    assert (m2.count, m2.lp_sum, m2.lp_sqsum) == (m.count, m.lp_sum, m.lp_sqsum)


# ---------------------------------------------------------------------------
# 7. high level
# ---------------------------------------------------------------------------

def test_high_level_api(cuda):
    flow = _flow("readme")
    x, lp = dfa.sample_logpdf(flow, (2, 5, 7), (1.25,), seed=7)
    assert tuple(x.shape) == (5, 2, 5, 7) and tuple(lp.shape) == (2, 5, 7)
    m = dfa.fisher_information(flow, (1.25,), 4096, chunk=1024, seed=7)
    assert m.fisher.shape == (1, 1) and m.count == 4096 and m.fisher[0, 0] > 0
    np.testing.assert_array_equal(m.fisher, m.fisher.T)
    # the same draws through sample and score_moments, chunk by chunk
    acc = np.zeros(5)
    for start, ln in _chunks(4096, 1024):
        xi = dfa.sample(flow, ln, (1.25,), seed=7, offset=5 * start // 4)
        mi = dfa.score_moments(flow, xi, (1.25,))
        acc = acc + np.concatenate([[mi.count, mi.lp_sum, mi.lp_sqsum], mi.score_sum, mi.outer.ravel(order="F")])
    got = np.concatenate([[m.count, m.lp_sum, m.lp_sqsum], m.score_sum, m.outer.ravel(order="F")])
    np.testing.assert_array_equal(_bits(got), _bits(acc))
    se = np.sqrt(max(m.score_cov[0, 0], 0.0) / m.count)
    print(f"readme: F = {m.fisher[0, 0]:.6g}, mean_score / stderr = {m.mean_score[0] / se:.3f}, "
          f"H = {m.entropy:.5f} ± {m.entropy_stderr:.5f}")
    # a live TrainState serves the calls, and df_chain_set_weights is not left blocked
    state = dfa.setup(Adam(), flow)
    with pytest.raises(_lib.ArgumentError, match="state="):
        dfa.fisher_information(flow, (1.25,), 64, seed=7)
    ms = dfa.fisher_information(flow, (1.25,), 4096, chunk=1024, seed=7, state=state)
    np.testing.assert_array_equal(_bits(ms.outer), _bits(m.outer))
    xi = dfa.sample(flow, 100, (1.25,), seed=7)
    a = dfa.score_moments(flow, xi, (1.25,), state=state)
    del state
    flow.hip().set_weights(flow.model.layers)
    b = dfa.score_moments(flow, xi, (1.25,))
    np.testing.assert_array_equal(_bits(a.outer), _bits(b.outer))
