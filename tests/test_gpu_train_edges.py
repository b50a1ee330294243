"""Training and score kernels past one trip of every batch loop ("training edge
matrix").

Every training kernel sizes a resident grid from the CU count and walks the batch in a
loop; on a whole chip a wave takes a second trip only past 32 768 samples, where no fp64
oracle gradient is a quick test.  `DF_GRID_CUS` (read at df_chain_create) sizes those grids
from 2 CUs here, so the second and third trips, the partial last one and the all-padding
waves beside it happen below 2 000 samples.  `DF_DEBUG_LAUNCH=1` makes df_train_create* and
the first df_train_logpdf_grad print the grids they planned; each test reads that line,
fails if the knob was not honoured, and takes every kernel's samples per trip P from it
(train_edge_cases.*_trips).  Batches: P − 1, P, P + 1, 2P + 17, 3P + 53 for every P of the
case's kernels (layer-wise: the front's 256 and ldense's 512, plus 1553), below 2 000.

Training, per case (train_edge_cases.CASES: one per kernel instance with a loop body of its
own, on the sweep form asserted from df_train_sweep) and batch:
  1. values: gradient and Σ logpdf against the fp64 oracle under test_gpu_train.py's
     criterion (1e-4 / 2e-5 per Dense tensor, loss to 1e-5).  A lost 16-sample tile misses it
     by a factor of 86 or more (tests/test_train_edges_host.py);
  2. poisoned tail: x and θ are prefixes of device buffers 2P + 7 rows longer whose further
     rows are NaN; the gradient must be finite;
  3. reused trainer: one trainer takes the largest batch and then every smaller one; each
     gradient is bitwise the one a fresh trainer gives (no stale masks, exp(−s), kept H, z̄);
  4. repeat: two evaluations are bitwise equal.
One more run per case at `DF_GRID_CUS=3` and the largest batch: an odd workgroup count and
dW ranges off the tile and 32-sample grids.

Score (df_train_logpdf_grad), per chain and batch: the per-sample outputs at 2 CUs are
bitwise those of an unforced trainer, pass test_gpu_score._check with that file's caps, and
leave the NaN pattern of 2P + 7 guard rows behind every output untouched.
"""
import re

import numpy as np
import pytest

import densityflows_amd.train as train_mod
import test_gpu_score as S
import train_edge_cases as T
from densityflows_amd import _lib
from densityflows_amd.train import Adam, HIPTrainer
from helpers import close, spec_to_element

pytestmark = pytest.mark.gpu

NAN32 = 0x7FC0DEAD                 # a quiet NaN with a recognisable payload
ENV_KEYS = ("DF_GRID_CUS", "DF_TILES", "DF_SMALL_MAX", "DF_SMALL_WAVES", "DF_F32_EXACT", "DF_NO_WIDE",
            "DF_FORCE_GENERIC", "DF_NO_FAST", "DF_NO_FOLD", "DF_SCORE_PER_NET", "DF_DEBUG_LAUNCH")
TRAIN_LINE = re.compile(r"\[df\] train: (\S+) sweep, (\d+) CUs \(of (\d+)\), grid (\d+) at (\d+) workgroups per CU, "
                        r"lgrid (\d+)")
SCORE_LINE = re.compile(r"\[df\] logpdf_grad: (\d+) launches \([^)]*\), (\d+) workgroups of (\d+) waves per CU, "
                        r"grid (\d+)")


def _trainer(chain, sweep, env, cus, monkeypatch, capfd):
    """A fresh chain and trainer (the plan reads the environment when the chain is created)
    and the grids df_train_create printed: (trainer, {sweep, cus, n_cu, grid, occ, lgrid})."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
    if cus:
        monkeypatch.setenv("DF_GRID_CUS", str(cus))
    capfd.readouterr()
    spec = T.case_data(chain)[0]
    tr = HIPTrainer(spec_to_element(spec).hip(), Adam(), sweep=getattr(train_mod, "SWEEP_" + sweep))
    lines = TRAIN_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, f"{chain}: expected one grid line from df_train_create, got {lines}"
    word, c, n_cu, grid, occ, lgrid = lines[0]
    return tr, dict(sweep=word, cus=int(c), n_cu=int(n_cu), grid=int(grid), occ=int(occ), lgrid=int(lgrid))


def _check_grids(info, cus, form, what):
    """The knob was honoured; returns the samples per trip of the case's kernels."""
    assert info["n_cu"] >= T.GRID_CUS_ODD, f"{what}: a device of {info['n_cu']} CUs cannot run this matrix"
    assert info["cus"] == cus, f"{what}: grids sized from {info['cus']} CUs, DF_GRID_CUS={cus}"
    assert info["occ"] >= 1
    if form == "FUSED":
        assert info["sweep"] == "fused" and info["grid"] == cus * info["occ"] and info["lgrid"] == 0, (what, info)
        return T.fused_trips(info["grid"])
    assert info["sweep"] == "layer-wise" and info["grid"] == cus and info["lgrid"] == cus, (what, info)
    return T.layerwise_trips(info["lgrid"])


def _poisoned(a, B, pad, dev):
    """The first B samples of a (rows, ·) followed by pad rows of NaN, flat, Julia order."""
    import torch

    rows = a.shape[0]
    buf = torch.full(((B + pad) * rows,), float("nan"), dtype=torch.float32, device=dev)
    buf[:B * rows] = torch.from_numpy(np.ascontiguousarray(a[:, :B].T).ravel()).to(dev)
    return buf


def _grad(tr, x, th, B, pad, dev):
    import torch

    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    xb = _poisoned(x, B, pad, dev)
    tb = _poisoned(th, B, pad, dev) if th.shape[0] else None
    tr.gradient(xb, tb, B, B, lp)
    torch.cuda.synchronize()
    return tr.grad().detach().cpu().numpy().copy(), float(lp.item())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _values(chain, spec, g, lpsum, B, what):
    """Property 1; returns the worst per-tensor violation ratio."""
    assert np.all(np.isfinite(g)) and np.isfinite(lpsum), f"{what}: non-finite gradient or Σ logpdf"
    loss, ref = T.oracle_grad(chain, B)
    assert g.shape == ref.shape
    assert abs(-lpsum / B - loss) <= 1e-5 * max(1.0, abs(loss)), f"{what}: loss {-lpsum / B} against {loss}"
    worst = max(close(g[sl], ref[sl], T.G_RTOL, T.G_ATOL)[1] for sl in T._tensor_slices(spec))
    assert worst <= 1.0, f"{what}: gradient violation ratio {worst}"
    return worst


@pytest.mark.parametrize("case", list(T.CASES))
def test_train_edges(cuda, case, monkeypatch, capfd):
    chain, sweep, form, env = T.CASES[case]
    spec, d, n, x, th = T.case_data(chain)
    want = getattr(train_mod, "SWEEP_" + form)
    make = lambda: _trainer(chain, sweep, env, T.GRID_CUS, monkeypatch, capfd)
    reused, info = make()
    assert reused.sweep() == want, f"{case}: sweep form {reused.sweep()}, expected {form}"
    trips = _check_grids(info, T.GRID_CUS, form, case)
    Bs = T.batches(trips, () if form == "FUSED" else T.LAYERWISE_EXTRA)
    Bmax, pad = Bs[-1], 2 * max(trips) + 7
    assert len(Bs) >= 3 and Bmax in T.largest_batches(form), (case, info, Bs)
    assert Bmax <= x.shape[1]

    worst = {}
    _grad(reused, x, th, Bmax, pad, cuda)
    for B in reversed(Bs):
        what = f"{case} B={B} ({info['grid']} workgroups)"
        fresh, finfo = make()
        assert finfo == info and fresh.sweep() == want, (what, finfo)
        g, lp = _grad(fresh, x, th, B, pad, cuda)
        worst[B] = _values(chain, spec, g, lp, B, what)
        g2, lp2 = _grad(fresh, x, th, B, pad, cuda)
        assert _same_bits(g, g2) and lp == lp2, f"{what}: two evaluations differ"
        assert fresh.sweep() == want
        gr, lpr = _grad(reused, x, th, B, pad, cuda)
        assert _same_bits(g, gr) and lp == lpr, \
            f"{what}: a trainer that ran B={Bmax} before differs from a fresh one ({int(np.sum(g != gr))} entries)"
    capfd.readouterr()
    print(f"TRAIN-EDGE {case}: {form} occ {info['occ']} grid {info['grid']} trips {trips} batches {Bs} "
          f"worst ratio {max(worst.values()):.3f} (at B={max(worst, key=worst.get)}; "
          + " ".join(f"{B}:{r:.3f}" for B, r in sorted(worst.items())) + ")")


@pytest.mark.parametrize("case", list(T.CASES))
def test_train_edges_odd_grid(cuda, case, monkeypatch, capfd):
    """`DF_GRID_CUS=3` at the largest batch of the case's matrix."""
    chain, sweep, form, env = T.CASES[case]
    spec, d, n, x, th = T.case_data(chain)
    tr, info = _trainer(chain, sweep, env, T.GRID_CUS_ODD, monkeypatch, capfd)
    assert tr.sweep() == getattr(train_mod, "SWEEP_" + form)
    _check_grids(info, T.GRID_CUS_ODD, form, case)
    # the batches and the pad of the two-CU matrix (same occupancy)
    trips = T.fused_trips(T.GRID_CUS * info["occ"]) if form == "FUSED" else T.layerwise_trips(T.GRID_CUS)
    B = T.batches(trips, () if form == "FUSED" else T.LAYERWISE_EXTRA)[-1]
    pad = 2 * max(trips) + 7
    what = f"{case} B={B} ({info['grid']} workgroups)"
    g, lp = _grad(tr, x, th, B, pad, cuda)
    worst = _values(chain, spec, g, lp, B, what)
    g2, lp2 = _grad(tr, x, th, B, pad, cuda)
    assert _same_bits(g, g2) and lp == lp2, f"{what}: two evaluations differ"
    capfd.readouterr()
    print(f"TRAIN-EDGE-ODD {case}: {form} grid {info['grid']} B {B} worst ratio {worst:.3f}")


def _guarded(rows, B, pad, dev):
    import torch

    return torch.full(((B + pad) * rows,), NAN32, dtype=torch.int32, device=dev).view(torch.float32)


def _take(buf, rows, B, what):
    """The B valid samples of a guarded buffer as (rows, B); the guard rows must still hold
    the pattern."""
    import torch

    raw = buf.view(torch.int32).cpu().numpy()
    assert np.all(raw[B * rows:] == NAN32), f"{what}: written past the batch (B = {B})"
    return raw[:B * rows].view(np.float32).reshape(B, rows).T.copy()


def _score(tr, x, th, B, pad, dev, what):
    """df_train_logpdf_grad on guarded outputs → (lp (B,), gx (d, B), gθ (n, B) or None)."""
    import torch

    d, n = x.shape[0], th.shape[0]
    lpb, gxb = _guarded(1, B, pad, dev), _guarded(d, B, pad, dev)
    gtb = _guarded(n, B, pad, dev) if n else None
    tr.logpdf_grad(S._dev(x[:, :B], dev), S._dev(th[:, :B], dev) if n else None, B, lpb, gxb, gtb)
    torch.cuda.synchronize()
    return (_take(lpb, 1, B, what + " lp")[0], _take(gxb, d, B, what + " gx"),
            _take(gtb, n, B, what + " gθ") if n else None)


def _score_line(capfd, what):
    lines = SCORE_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, f"{what}: expected one grid line from the first df_train_logpdf_grad, got {lines}"
    launches, occ, waves, grid = (int(v) for v in lines[0])
    return occ, waves, grid


@pytest.mark.parametrize("name", list(T.SCORE_CASES))
def test_score_edges(cuda, name, monkeypatch, capfd):
    cap = T.SCORE_CASES[name]
    spec, x, th, ref = T.score_data(name)
    forced, info = _trainer(name, "AUTO", {}, T.GRID_CUS, monkeypatch, capfd)
    base, binfo = _trainer(name, "AUTO", {}, 0, monkeypatch, capfd)
    assert info["cus"] == T.GRID_CUS and binfo["cus"] == binfo["n_cu"] >= T.GRID_CUS_ODD, (info, binfo)
    for tr in (forced, base):
        tr.set_theta_input(_lib.DF_THETA_GIVEN)
    # the launches are planned (and printed) by the first call
    _score(forced, x, th, 17, 7, cuda, f"{name} first call")
    occ, waves, grid = _score_line(capfd, name)
    assert waves == 4 and occ >= 1 and grid == T.GRID_CUS * occ, f"{name}: score grid {grid} at {occ} per CU"
    _score(base, x, th, 17, 7, cuda, f"{name} first call, unforced")
    bocc, _, bgrid = _score_line(capfd, name + " unforced")
    assert bocc == occ and bgrid == binfo["n_cu"] * occ, f"{name}: unforced score grid {bgrid} at {bocc} per CU"

    trips = T.score_trips(grid)
    Bs, pad = T.batches(trips), 2 * trips[0] + 7
    assert len(Bs) >= 3, (name, occ, Bs)
    for B in Bs:
        what = f"{name} B={B} ({grid} workgroups)"
        got = _score(forced, x, th, B, pad, cuda, what)
        want = _score(base, x, th, B, pad, cuda, what + " unforced")
        for q, a, b in zip(("lp", "gx", "gθ"), got, want):
            assert (a is None and b is None) or _same_bits(a, b), f"{what}: {q} differs from the unforced trainer's"
        gth = got[2] if got[2] is not None else np.zeros((0, B), np.float32)
        S._check((got[0], got[1], gth), (ref[0][:B], ref[1][:, :B], ref[2][:, :B], ref[3][:B]), cap, what)
    capfd.readouterr()
    print(f"SCORE-EDGE {name}: occ {occ} grid {grid} trips {trips} batches {Bs}")
