"""Marginal tables on the device (df_flow_pdf_marginals, flows.pdf_marginals): the grid's pdf
reduced chunk by chunk into 0-, 1- and 2-D tables, in fp64.

Two references, both through tests/marginal_ref.py (pinned in test_marginals_host.py):
the case's OWN ``logpdf_grid`` values cast to fp64, which the tables must match to fp64
rounding — a dropped point, a wrong bin or a wrong excluded weight cannot hide under the
chain's tolerance there — and the fp64 oracle, under the bound the project's close(·, 1e-5)
criterion on logpdf implies for a weighted sum of pdf values.  The grids are those of
tests/grid_cases.py; every request list is the full one ((), all singles, all pairs) unless
the test says otherwise; every run uses chunk 0 and chunk 64.  Output buffers are 8 doubles
longer than the tables and pre-filled with one NaN bit pattern that must survive.

The 1e-12 relative bound of the exact checks is derived, not measured: the trapezoid
weights on these quantile axes are positive (asserted), so all terms of a bin are
non-negative and the error of its sum is at most (terms per bin ≤ 1260) · 2⁻⁵³ ≈ 1.4e-13
relative, plus the two ulps by which two correctly working ``exp`` may differ and the
roundings of at most 8 weight products."""
import numpy as np
import pytest

import densityflows_amd as dfa
import grid_cases as G
import marginal_ref as M
from densityflows_amd import _lib
from test_gpu_grid import _Case, _flat, _kernels, _same_bits

pytestmark = pytest.mark.gpu

NAN64 = 0x7FF8DEADBEEF0000
PAD = 8
RTOL = 1e-5              # the chain's criterion on logpdf (helpers.close)
EXACT = 1e-12


def _weights(g, rule="trapezoid"):
    axes = g["x_axes"] + g["th_axes"]
    return [dfa.trapezoid_weights(a) if rule == "trapezoid" else np.ones(len(a)) for a in axes]


def _run(C, g, weights, keeps, first, count, chunk, lens=None, out=None):
    """df_flow_pdf_marginals into a guarded buffer → {keep: table} (pad checked).  ``out``: the
    buffer of a call that the library must refuse."""
    import torch

    lens = g["lens"] if lens is None else lens
    wbuf = None if weights is None else torch.from_numpy(np.concatenate(weights)).to(C.dev)
    if out is not None:         # a call that must be refused: the caller checks `out` afterwards
        C.h.run_pdf_marginals(C.axes_buf(g), wbuf, lens, first, count, keeps, out.view(torch.float64), chunk)
        raise AssertionError(f"{C.name}: the call was not refused")
    shapes = [M.table_shape(lens, K) for K in keeps]
    sizes = [int(np.prod(s, dtype=np.int64)) for s in shapes]
    total = sum(sizes)
    out = torch.full((total + PAD,), NAN64, dtype=torch.int64, device=C.dev)
    C.h.run_pdf_marginals(C.axes_buf(g), wbuf, lens, first, count, keeps, out.view(torch.float64), chunk)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[total:] == NAN64), f"{C.name}: written past the {total} table values"
    res, at = {}, 0
    for K, shape, size in zip(keeps, shapes, sizes):
        res[K] = raw[at:at + size].view(np.float64).reshape(shape, order="F").copy()
        at += size
    return res


def _assert_close(got, want, tol, what):
    """Per bin |got − want| ≤ tol (an array or a scalar); prints the worst ratio."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), what
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    err = np.abs(got - want)
    bad = err > tol
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0)))) if want.size else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} bins out of tolerance, worst ratio {worst:.3g}"
    return worst


def _oracle_bound(g, weights, K):
    """Σ |c_p| · expm1(τ_p) per bin, τ_p the close(·, 1e-5) tolerance of point p's logpdf."""
    lp = np.asarray(g["lp"], np.float64)
    tau = RTOL * max(1.0, float(np.max(np.abs(lp)))) + RTOL * np.abs(lp)
    return M.marginal(np.exp(lp) * np.expm1(tau), g["lens"], [np.abs(w) for w in weights], K)


TABLE_CASES = [("split64", G.LENS5, None), ("split64", G.LENS_MANY, None), ("fast16", G.LENS5, None),
               (G.README16, G.LENS5, None), ("norm_only_d5", G.LENS5, None),
               ("slowcopy_d12", G.LENS_X[12], None),                    # more than 8 axes: the 64-slot kernel
               ("wide_split", G.LENS_X[6], G.THETA_AXES["wide_split"]),
               ("split32", G.LENS_X[5], G.THETA_AXES["split32"])]


@pytest.mark.parametrize("name,lens_x,lens_th", TABLE_CASES,
                         ids=[f"{c[0]}-{int(np.prod(c[1]))}" + ("-theta" if c[2] else "") for c in TABLE_CASES])
def test_tables_exact_and_against_the_oracle(cuda, name, lens_x, lens_th, monkeypatch):
    """Check 1: every table equals marginal_ref of the case's own logpdf_grid values within
    1e-12 relative per bin.  Check 2: against the fp64 oracle, per bin
    |m_gpu − m_oracle| ≤ Σ |c_p| · expm1(τ_p) + 1e-12 · |m_oracle|."""
    C = _Case(name, monkeypatch, cuda)
    g = G.grid_data(name, lens_x, lens_th)
    P, lens = g["x"].shape[1], g["lens"]
    w = _weights(g)
    assert all(np.all(x > 0) for x in w)
    keeps = M.all_requests(len(lens))
    if len(keeps) > 128:        # 21 axes: the total, all singles, the pairs among seven axes (two of them θ)
        keeps = [K for K in keeps if len(K) < 2 or set(K) <= {0, 2, 4, 6, 11, 12, 20}]
    assert len(keeps) <= 128 and P <= 1260
    own = M.marginals_of_logpdf(C.grid(g, 0, P, 0), lens, w, keeps)
    oracle = M.marginals_of_logpdf(g["lp"], lens, w, keeps)
    for chunk in (0, 64):
        got = _run(C, g, w, keeps, 0, P, chunk)
        r1 = max(_assert_close(got[K], own[K], EXACT * np.abs(own[K]), f"{name} {K} chunk {chunk}, exact")
                 for K in keeps)
        r2 = max(_assert_close(got[K], oracle[K], _oracle_bound(g, w, K) + EXACT * np.abs(oracle[K]),
                               f"{name} {K} chunk {chunk}, oracle") for K in keeps)
        print(f"MARGINALS {name} {P} points chunk {chunk}: {len(keeps)} tables, worst ratio exact {r1:.3g}, "
              f"oracle {r2:.3g}")


def test_windows_add_up(cuda, monkeypatch):
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", G.LENS5)
    P, w, keeps = g["x"].shape[1], _weights(g), M.all_requests(len(g["lens"]))
    full = _run(C, g, w, keeps, 0, P, 0)
    parts = [_run(C, g, w, keeps, a, b - a, chunk) for (a, b), chunk in zip(((0, 100), (100, 163), (163, P)),
                                                                            (0, 64, 0))]
    for K in keeps:
        _assert_close(sum(p[K] for p in parts), full[K], EXACT * np.abs(full[K]), f"windows {K}")


@pytest.mark.parametrize("lens_x,first", [(G.HUGE_LENS, G.HUGE_FIRST), ((G.BIG_LEN,) * 5, G.BIG_FIRST)],
                         ids=["strides-2^32", "window-2^33"])
def test_64_bit_arithmetic(cuda, lens_x, first, monkeypatch):
    """A 300-point window of a grid of 2³⁵ points and more, strides past 32 bits: the tables
    of the window's own logpdf values, and every bin the window does not reach exactly 0.
    The (0,) table of the first grid has 65,536 bins: larger than the LDS budget."""
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", lens_x, None, first, G.BIG_COUNT)
    lens, w = g["lens"], _weights(g)
    assert all(np.all(x >= 0) for x in w)              # 65,536 quantiles of one sample: neighbours may coincide
    keeps = [(), (0,), (2,), (3,), (4,), (3, 4)]
    lp = C.grid(g, first, G.BIG_COUNT, 0)
    own = M.marginals_of_logpdf(lp, lens, w, keeps, first)
    assert own[(0,)].shape == (lens[0],) and np.count_nonzero(own[(0,)]) <= G.BIG_COUNT
    for chunk in (0, 64):
        got = _run(C, g, w, keeps, first, G.BIG_COUNT, chunk)
        for K in keeps:
            _assert_close(got[K], own[K], EXACT * np.abs(own[K]), f"{K} chunk {chunk}")
            assert np.array_equal(got[K] == 0.0, own[K] == 0.0), f"{K}: a bin outside the window was touched"
            assert not np.any(np.signbit(got[K]))


def test_table_larger_than_lds_with_every_bin_hit(cuda, monkeypatch):
    """A 200 × 150 table (30,000 bins, the LDS budget is 6,144) on a grid of as many points:
    every bin gets exactly one term, so the bound is that of one product: two ulps of exp and
    the roundings of three weights, below 1e-14 relative.  The (0,) and (1,) tables of the same
    call go through LDS, 150 and 200 terms per bin."""
    C = _Case("split64", monkeypatch, cuda)
    lens = (200, 150, 1, 1, 1, 1)
    xa, ta = G.case_axes("split64", lens[:5])
    g = dict(x_axes=xa, th_axes=ta, lens=lens)
    w = _weights(g)
    assert all(np.all(x > 0) for x in w)
    P = 30000
    keeps = [(0, 1), (0,), (1,), ()]
    lp = C.grid(g, 0, P, 0)
    own = M.marginals_of_logpdf(lp, lens, w, keeps)
    assert np.all(own[(0, 1)] > 0)
    for chunk in (0, 64):
        got = _run(C, g, w, keeps, 0, P, chunk)
        _assert_close(got[(0, 1)], own[(0, 1)], 1e-14 * own[(0, 1)], f"(0, 1) chunk {chunk}")
        for K in keeps[1:]:
            _assert_close(got[K], own[K], EXACT * np.abs(own[K]), f"{K} chunk {chunk}")


def test_callers_weights_of_mixed_sign(cuda, monkeypatch):
    """Weights of both signs and a zero: cancellation makes a relative bound meaningless, so a
    bin is judged on its absolute scale, 1e-12 · Σ |c_p|."""
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", G.LENS5)
    P, lens = g["x"].shape[1], g["lens"]
    rng = np.random.default_rng(5)
    w = [rng.normal(size=L) for L in lens]
    w[2][3] = 0.0                                   # a zero on axis 2, kept by some requests and not by others
    w[1][0] = -2.5                                  # the length-1 axis carries a weight too
    assert any(np.any(x < 0) for x in w) and any(np.any(x > 0) for x in w)
    keeps = M.all_requests(len(lens))
    lp = C.grid(g, 0, P, 0)
    own = M.marginals_of_logpdf(lp, lens, w, keeps)
    scale = {K: M.marginal(np.exp(lp.astype(np.float64)), lens, [np.abs(x) for x in w], K) for K in keeps}
    for chunk in (0, 64):
        got = _run(C, g, w, keeps, 0, P, chunk)
        for K in keeps:
            _assert_close(got[K], own[K], EXACT * scale[K], f"{K} chunk {chunk}")


def test_output_guard_and_handle_state(cuda, monkeypatch, capfd):
    import torch

    C = _Case("split64", monkeypatch, cuda)
    flow, g = C.flow(), G.grid_data("split64", G.LENS5)
    P, h, lens = g["x"].shape[1], C.h, g["lens"]
    w, keeps = _weights(g), M.all_requests(len(g["lens"]))
    xb, tb = _flat(g["x"], cuda), _flat(g["th_raw"], cuda)
    th = tuple(float(a[0]) for a in g["th_axes"])

    def state():
        lp = torch.empty(P, dtype=torch.float32, device=cuda)
        h.run_logpdf(xb, tb, lp, P)
        smp = dfa.sample(flow, (3, 50), th, seed=12345, offset=7)
        torch.cuda.synchronize()
        return lp.cpu().numpy(), smp.cpu().numpy(), C.grid(g, 0, P, 64)

    before = state()
    capfd.readouterr()
    # count == 0: the tables are zeroed (they were NaN), the pad is not, nothing is launched
    for first in (0, P):
        z = _run(C, g, w, keeps, first, 0, 0)
        assert all(np.all(t == 0.0) and not np.any(np.signbit(t)) for t in z.values())
    lens0 = list(lens)
    lens0[2] = 0                                                    # an empty axis: empty tables among the zeroed
    z = _run(C, g, w, keeps, 0, 0, 64, lens=lens0)
    assert z[(2,)].shape == (0,) and z[(0, 2)].shape == (3, 0) and z[()] == 0.0 and np.all(z[(0, 4)] == 0.0)
    # no request: nothing runs, nothing is written
    assert _run(C, g, w, [], 0, P, 0) == {}
    assert _kernels(capfd) == []
    # the refusals
    room = torch.full((4096,), NAN64, dtype=torch.int64, device=cuda)
    for bad in ([(6,)], [(-2,)], [(2, 2)], [(4, 1)], [(0, 6)]):
        with pytest.raises(_lib.ArgumentError):
            _run(C, g, w, bad, 0, P, 0, out=room)
    with pytest.raises(_lib.ArgumentError):
        _run(C, g, None, keeps, 0, P, 0, out=room)                  # null weights
    with pytest.raises(_lib.UnsupportedError):
        _run(C, g, w, [()] * 129, 0, P, 0, out=room)
    for first, count in ((0, P + 1), (P, 1), (-1, 2), (0, -1), (1, 2**63 - 1)):
        with pytest.raises(_lib.DimensionMismatch):
            _run(C, g, w, keeps, first, count, 0, out=room)
    with pytest.raises(_lib.DimensionMismatch):
        _run(C, g, w, [()], 0, 1, 0, lens=[3, 1, -5, 2, 7, 1], out=room)
    with pytest.raises(_lib.DimensionMismatch):
        _run(C, g, w, [()], 0, 1, 0, lens=[2**31] * 5 + [1], out=room)       # P past int64
    with pytest.raises(_lib.DimensionMismatch):
        _run(C, g, w, [(0, 1)] * 3, 0, 0, 0, lens=[2**31, 2**31, 0, 1, 1, 1], out=room)   # 3 · 2⁶² bins
    assert _kernels(capfd) == []
    assert np.all(room.cpu().numpy() == NAN64)
    # a second identical call: the same sums, up to the order the atomic adds arrived in
    a = _run(C, g, w, keeps, 0, P, 64)
    b = _run(C, g, w, keeps, 0, P, 64)
    for K in keeps:
        _assert_close(b[K], a[K], 1e-13 * np.abs(a[K]), f"second call {K}")
    _run(C, g, w, keeps, 0, P, 0)
    # marginal calls (staging grown twice) leave the handle's other entry points as they were
    after = state()
    for x, y, what in zip(after, before, ("logpdf", "sample", "logpdf_grid")):
        _same_bits(x, y, f"{what} after marginal calls")


def test_public_api(cuda, monkeypatch):
    import torch

    C = _Case("split64", monkeypatch, cuda)
    flow, g = C.flow(), G.grid_data("split64", G.LENS5)
    P, lens = g["x"].shape[1], g["lens"]
    axes, th = tuple(g["x_axes"]), tuple(float(a[0]) for a in g["th_axes"])
    w = _weights(g)
    res = dfa.pdf_marginals(flow, axes, th)
    # the corner: the total mass, the x axes of more than one value, their pairs; keys sorted
    assert list(res) == [(), (0,), (2,), (3,), (4,), (0, 2), (0, 3), (0, 4), (2, 3), (2, 4), (3, 4)]
    own = M.marginals_of_logpdf(C.grid(g, 0, P, 0), lens, w, list(res))
    for K, t in res.items():
        assert isinstance(t, np.ndarray) and t.dtype == np.float64 and t.shape == M.table_shape(lens, K)
        assert t.flags.f_contiguous
        _assert_close(t, own[K], EXACT * np.abs(own[K]), f"pdf_marginals {K}")
    # keep in any order, θ axes among the kept, θ entries as values or vectors; a window
    part = dfa.pdf_marginals(flow, axes, (np.array(th[:1], np.float32),) + th[1:], keep=[(5, 2), (4,), (2, 5)],
                             first=10, count=150, chunk=64)
    assert list(part) == [(4,), (2, 5)] and part[(2, 5)].shape == (5, 1)
    ref = M.marginals_of_logpdf(C.grid(g, 10, 150, 0), lens, w, list(part), first=10)
    for K in part:
        _assert_close(part[K], ref[K], EXACT * np.abs(ref[K]), f"window {K}")
    # weights="sum" is the plain sum of pdf: pdf takes exp in fp32, hence 1e-6
    p32 = dfa.pdf(flow, axes, th)
    assert p32.dtype == np.float32 and p32.shape == G.LENS5
    summed = dfa.pdf_marginals(flow, axes, th, keep=[(), (2,), (0, 4)], weights="sum")
    p64 = p32.astype(np.float64)
    for K, want in (((), p64.sum()), ((2,), p64.sum(axis=(0, 1, 3, 4))), ((0, 4), p64.sum(axis=(1, 2, 3)))):
        _assert_close(summed[K], np.asarray(want), 1e-6 * np.abs(want), f"weights=sum {K}")
    # the caller's own rule
    mine = dfa.pdf_marginals(flow, axes, th, keep=[(0,)], weights=tuple(2.0 * x for x in w))
    _assert_close(mine[(0,)], 32.0 * own[(0,)], 32.0 * EXACT * np.abs(own[(0,)]), "weights tuple")
    # device axes in, device tensors out, the same values
    dres = dfa.pdf_marginals(flow, tuple(torch.from_numpy(np.array(a)).to(cuda) for a in axes), th)
    assert list(dres) == list(res)
    for K, t in dres.items():
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.float64
        assert tuple(t.shape) == M.table_shape(lens, K)
        _assert_close(t.cpu().numpy(), res[K], 1e-13 * np.abs(res[K]), f"device axes {K}")
    # the three error classes
    with pytest.raises(_lib.DimensionMismatch):
        dfa.pdf_marginals(flow, axes[:4], th)
    with pytest.raises(_lib.DimensionMismatch):
        dfa.pdf_marginals(flow, axes, th, weights=tuple(w[:-1]))
    with pytest.raises(_lib.DimensionMismatch):
        dfa.pdf_marginals(flow, axes, th, first=P - 3, count=4)
    with pytest.raises(_lib.UnsupportedError):
        dfa.pdf_marginals(flow, axes, th, keep=[(0, 2, 4)])
    with pytest.raises(_lib.ArgumentError):
        dfa.pdf_marginals(flow, axes, th, keep=[(0, 6)])
    with pytest.raises(_lib.ArgumentError):
        dfa.pdf_marginals(flow, axes, th, weights="simpson")
