"""Device-resident epochs on the GPU: df_batch_gather against numpy.take, df_train_epoch
against a Python loop of df_train_step on host-gathered batches (bitwise: the same kernels
with the same arguments in the same order), train_(loader="device") against
train_(loader="host"), and the order check."""
import ctypes as C

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.train import (SWEEP_FUSED, SWEEP_LAYERWISE, Adam, ClipNorm, HIPTrainer, OptimiserChain,
                                    load_trainables, setup, train_, trainables)
from helpers import spec_to_element
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

CANARY = np.float32(-12345.5)


def _readme_spec(rng):
    """test/runtests.jl:103-109: three RNVP layers (d = 5, n = 1, hidden 16) + NormalizationLayer."""
    layers = [O.rnvp_layer(rng, O.coupling_axes(5, m, n=1), hidden=16, bias_scale=0.1, out_scale=0.5)
              for m in ([1, 2, 3], [3, 4, 5], [5, 1, 2])]
    layers.append({"kind": "norm", "x_min": np.full(5, -3.0, np.float32), "x_max": np.full(5, 2.5, np.float32),
                   "alpha": -1.0, "beta": 1.0})
    return {"kind": "chain", "layers": layers}


def _block_spec(rng):
    """An unconditional d = 5 chain of two hidden-64 CouplingBlocks (θ is a null pointer)."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(5, 2, n=0), hidden=64, bias_scale=0.1, out_scale=0.3),
        O.coupling_block(rng, O.coupling_axes_cut(5, 3, n=0), hidden=64, bias_scale=0.1, out_scale=0.3),
    ]}


def _dev(a, dev):
    """numpy (rows, B) → flat Julia-order device buffer (None for no rows)."""
    import torch

    a = np.asarray(a, np.float32)
    if a.shape[0] == 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)


def _set(d, n, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d, N)).astype(np.float32)
    th = rng.random((n, N)).astype(np.float32)
    return x, th


# ---- 1. df_batch_gather -----------------------------------------------------------------

N_SET = 7 + 257          # first = 7 with count = 257 ends exactly at the set's last sample


@pytest.mark.parametrize("d,n", [(5, 1), (1, 0), (32, 8), (3, 61)])
def test_gather_matches_numpy_take(cuda, d, n):
    """Every (count, first, order) against numpy.take, bitwise; three canary rows past `count`
    in each output stay as they were."""
    import torch

    lib = _lib.load()
    x, th = _set(d, n, N_SET, seed=d * 100 + n)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    rng = np.random.default_rng(3)
    rep = rng.integers(0, N_SET, N_SET).astype(np.int32)       # with repeats (and so with gaps)
    assert len(np.unique(rep)) < N_SET
    orders = {"repeats": (rep, torch.from_numpy(rep).to(cuda)), "null": (np.arange(N_SET), None)}
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    runs = []
    for count in (1, 63, 64, 65, 257):
        for first in (0, 7):
            if first + count > N_SET:
                continue
            for name, (oh, od) in orders.items():
                xo = torch.full(((count + 3) * d,), float(CANARY), dtype=torch.float32, device=cuda)
                to = torch.full(((count + 3) * n,), float(CANARY), dtype=torch.float32, device=cuda) if n else None
                rc = lib.df_batch_gather(ptr(xo), ptr(to), ptr(xs), ptr(ts), d, n, N_SET, ptr(od), first, count, stream)
                assert rc == _lib.DF_OK, lib.df_last_error()
                runs.append((count, first, name, oh[first:first + count], xo, to))
    assert any(f + c == N_SET for c, f, *_ in runs)
    torch.cuda.synchronize()
    for count, first, name, idx, xo, to in runs:
        tag = f"count={count} first={first} order={name}"
        got = xo.cpu().numpy().reshape(count + 3, d)
        np.testing.assert_array_equal(got[:count].view(np.int32), np.take(x, idx, axis=1).T.view(np.int32), err_msg=tag)
        assert np.all(got[count:] == CANARY), tag
        if n:
            got = to.cpu().numpy().reshape(count + 3, n)
            np.testing.assert_array_equal(got[:count].view(np.int32), np.take(th, idx, axis=1).T.view(np.int32),
                                          err_msg=tag)
            assert np.all(got[count:] == CANARY), tag


def test_gather_of_nothing_writes_nothing_and_windows_are_checked(cuda):
    import torch

    lib = _lib.load()
    x, th = _set(5, 1, 16, seed=1)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    xo = torch.full((20,), float(CANARY), dtype=torch.float32, device=cuda)
    to = torch.full((4,), float(CANARY), dtype=torch.float32, device=cuda)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert lib.df_batch_gather(ptr(xo), ptr(to), ptr(xs), ptr(ts), 5, 1, 16, None, 16, 0, stream) == _lib.DF_OK
    # a window that leaves the set is refused before any launch
    assert lib.df_batch_gather(ptr(xo), ptr(to), ptr(xs), ptr(ts), 5, 1, 16, None, 14, 3, stream) == _lib.DF_ERR_INVALID
    assert lib.df_batch_gather(ptr(xo), ptr(to), ptr(xs), ptr(ts), 5, 1, 16, None, -1, 2, stream) == _lib.DF_ERR_INVALID
    assert lib.df_batch_gather(ptr(xo), ptr(to), ptr(xs), ptr(ts), 5, 1, 1 << 31, None, 0, 2, stream) == _lib.DF_ERR_SHAPE
    torch.cuda.synchronize()
    assert np.all(xo.cpu().numpy() == CANARY) and np.all(to.cpu().numpy() == CANARY)


def test_trainer_gather(cuda):
    """HIPTrainer.gather takes d and n from its chain."""
    import torch

    chain = spec_to_element(_readme_spec(np.random.default_rng(0)))
    tr = HIPTrainer(chain.hip(), Adam())
    x, th = _set(5, 1, 40, seed=2)
    order = np.random.default_rng(4).permutation(40).astype(np.int32)
    xo = torch.empty(9 * 5, dtype=torch.float32, device=cuda)
    to = torch.empty(9, dtype=torch.float32, device=cuda)
    tr.gather(xo, to, _dev(x, cuda), _dev(th, cuda), 40, torch.from_numpy(order).to(cuda), 31, 9)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xo.cpu().numpy().reshape(9, 5), x[:, order[31:]].T)
    np.testing.assert_array_equal(to.cpu().numpy().reshape(9, 1), th[:, order[31:]].T)


# ---- 2. df_train_epoch against the step loop ---------------------------------------------

def _pair(make, opt, sweep):
    """Two trainers from the same seeded parameters (a trainer repacks its chain: one chain each)."""
    out = []
    for _ in range(2):
        chain = spec_to_element(make(np.random.default_rng(11)))
        out.append((chain, HIPTrainer(chain.hip(), opt(), sweep)))
    np.testing.assert_array_equal(out[0][1].get_params(), out[1][1].get_params())
    return out[0][1], out[1][1], out


def _loop_epoch(tr, x, th, order, bs, dev):
    """The epoch as a host loop: tr.step on host-gathered batches; returns every step's Σ logpdf."""
    import torch

    N = x.shape[1]
    lps = []
    for b0 in range(0, N, bs):
        idx = order[b0:b0 + bs]
        lp = torch.zeros(1, dtype=torch.float64, device=dev)
        tr.step(_dev(x[:, idx], dev), _dev(th[:, idx], dev), idx.shape[0], lpsum=lp)
        lps.append(lp)
    torch.cuda.synchronize()
    return np.array([float(lp.item()) for lp in lps])


def _epochs_match(cuda, make, d, n, N, bs, opt=Adam, sweep=None, epochs=3, between=None, fused=None):
    """`epochs` epochs (a fresh permutation each, in buffers that stay where they are, so the
    second sight of a step is captured and later ones replay) on both trainers; parameters
    and per-step Σ logpdf bitwise after every epoch."""
    import torch

    dev_tr, loop_tr, keep = _pair(make, opt, sweep)
    if fused is not None:
        assert (dev_tr.sweep() == SWEEP_FUSED) == fused
    x, th = _set(d, n, N, seed=N + bs)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    steps = -(-N // bs)
    od = torch.empty(N, dtype=torch.int32, device=cuda)
    slp = torch.zeros(steps, dtype=torch.float64, device=cuda)
    rng = np.random.default_rng(5)
    for ep in range(epochs):
        if between is not None and ep > 0:
            between(dev_tr)
            between(loop_tr)
        order = rng.permutation(N).astype(np.int32)
        od.copy_(torch.from_numpy(order))
        slp.fill_(float("nan"))
        assert dev_tr.epoch(xs, ts, N, od, bs, slp) == steps
        ref = _loop_epoch(loop_tr, x, th, order, bs, cuda)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(slp.cpu().numpy().view(np.int64), ref.view(np.int64), err_msg=f"epoch {ep}")
        np.testing.assert_array_equal(dev_tr.get_params().view(np.int32), loop_tr.get_params().view(np.int32),
                                      err_msg=f"epoch {ep}")
        assert np.all(np.isfinite(ref))
    return dev_tr, loop_tr, (x, th, xs, ts)


@pytest.mark.parametrize("N,bs", [(150, 64), (128, 64), (150, 150), (40, 1000), (3, 1)])
def test_epoch_equals_step_loop(cuda, N, bs):
    _epochs_match(cuda, _readme_spec, 5, 1, N, bs, fused=True)


def test_epoch_equals_step_loop_layerwise(cuda):
    _epochs_match(cuda, _readme_spec, 5, 1, 150, 64, sweep=SWEEP_LAYERWISE, fused=False)


def test_epoch_equals_step_loop_unconditional_blocks(cuda):
    _epochs_match(cuda, _block_spec, 5, 0, 150, 64)


def test_epoch_equals_step_loop_with_clipnorm_chain(cuda):
    _epochs_match(cuda, _readme_spec, 5, 1, 150, 64, opt=lambda: OptimiserChain(ClipNorm(1.0), Adam(1e-3)))


def test_adjust_between_epochs_recaptures(cuda):
    """adjust! after the steps were captured: a stale replay would keep η = 1e-3."""
    import torch

    etas = {}

    def between(tr):
        etas.setdefault(id(tr), iter([5e-4, 2.5e-4, 1e-4]))
        tr.adjust(next(etas[id(tr)]))

    dev_tr, loop_tr, (x, th, xs, ts) = _epochs_match(cuda, _readme_spec, 5, 1, 150, 64, epochs=4, between=between)
    # and it did change the step: a trainer that never adjusts ends elsewhere
    _, plain, _ = _pair(_readme_spec, Adam, None)
    rng = np.random.default_rng(5)
    for _ in range(4):
        _loop_epoch(plain, x, th, rng.permutation(150).astype(np.int32), 64, cuda)
    assert not np.array_equal(plain.get_params(), dev_tr.get_params())


def test_epoch_without_an_order_and_without_step_losses(cuda):
    """order = None: the set's own order, no synchronisation; step_lp = None."""
    import torch

    dev_tr, loop_tr, _ = _pair(_readme_spec, Adam, None)
    x, th = _set(5, 1, 150, seed=9)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    for _ in range(3):
        assert dev_tr.epoch(xs, ts, 150, None, 64) == 3
        _loop_epoch(loop_tr, x, th, np.arange(150), 64, cuda)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev_tr.get_params(), loop_tr.get_params())


def test_epoch_argument_errors(cuda):
    import torch

    chain = spec_to_element(_readme_spec(np.random.default_rng(0)))
    tr = HIPTrainer(chain.hip(), Adam())
    p0 = tr.get_params().copy()
    x, th = _set(5, 1, 8, seed=1)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    assert tr.epoch(xs, ts, 0, None, 4) == 0                    # nothing runs
    with pytest.raises(_lib.ArgumentError):
        tr.epoch(xs, ts, 8, None, 0)
    with pytest.raises(_lib.ArgumentError):
        tr.epoch(xs, ts, 8, None, -3)
    with pytest.raises(_lib.ArgumentError):
        tr.epoch(None, ts, 8, None, 4)
    with pytest.raises(_lib.DimensionMismatch):
        tr.epoch(xs, ts, 1 << 31, None, 4)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tr.get_params(), p0)


# ---- 3. order validation ------------------------------------------------------------------

def test_bad_order_is_refused_before_any_step(cuda):
    """An order holding N and -1: DF_ERR_INVALID naming two entries, the parameters bitwise
    unchanged (the check runs before any gather, so no kernel reads out of range), and the
    trainer runs a correct epoch afterwards."""
    import torch

    N, bs = 150, 64
    dev_tr, loop_tr, _ = _pair(_readme_spec, Adam, None)
    p0 = dev_tr.get_params().copy()
    x, th = _set(5, 1, N, seed=21)
    xs, ts = _dev(x, cuda), _dev(th, cuda)
    order = np.random.default_rng(8).permutation(N).astype(np.int32)
    bad = order.copy()
    bad[10], bad[140] = N, -1
    od = torch.from_numpy(bad).to(cuda)
    slp = torch.zeros(3, dtype=torch.float64, device=cuda)
    with pytest.raises(_lib.ArgumentError, match=r"\b2 of the 150 order entries"):
        dev_tr.epoch(xs, ts, N, od, bs, slp)
    assert dev_tr.steps_done == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev_tr.get_params().view(np.int32), p0.view(np.int32))
    assert np.all(slp.cpu().numpy() == 0.0)
    od.copy_(torch.from_numpy(order))
    assert dev_tr.epoch(xs, ts, N, od, bs, slp) == 3
    ref = _loop_epoch(loop_tr, x, th, order, bs, cuda)
    np.testing.assert_array_equal(slp.cpu().numpy(), ref)
    np.testing.assert_array_equal(dev_tr.get_params(), loop_tr.get_params())


# ---- 4. train_ end to end -----------------------------------------------------------------

def _flow(scale=1.0):
    """N_train = 150, N_valid = 40 of a synthetic (5, 190) set with one condition; the README
    chain with seeded weights, all trainables times `scale`."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal((5, 190)).astype(np.float32)
    th = (rng.random((1, 190)) * 4.0 - 1.0).astype(np.float32)
    data = dfa.DataArrays(x, th, f_training=150 / 190, f_validation=40 / 190, rng=rng)
    chain = dfa.FlowChain(
        dfa.CouplingLayer(data, [1, 2, 3], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.CouplingLayer(data, [3, 4, 5], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.CouplingLayer(data, [5, 1, 2], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.NormalizationLayer.from_data(x, -1.0, 1.0))
    if scale != 1.0:
        load_trainables(chain, trainables(chain) * np.float32(scale))
    flow = dfa.Flow(chain, data)
    assert data.training_data()[0].shape[1] == 150 and data.validation_data()[0].shape[1] == 40
    return data, chain, flow


def test_train_device_loader_equals_host_loader(cuda):
    import torch

    out = {}
    for loader in ("host", "device"):
        data, chain, flow = _flow()
        state = setup(Adam(1e-3), flow)
        if loader == "device":
            p0 = state.trainer.get_params().copy()
        kw = dict(return_step_losses=True) if loader == "device" else {}
        r = train_(flow, data, state, epochs=3, batchsize=64, shuffle=True, verbose=False,
                   rng=np.random.default_rng(7), loader=loader, **kw)
        out[loader] = (state.trainer.get_params(), trainables(chain), list(flow.train_loss), list(flow.valid_loss), r)
    h, dv = out["host"], out["device"]
    assert h[4] is None
    np.testing.assert_array_equal(dv[0].view(np.int32), h[0].view(np.int32))
    np.testing.assert_array_equal(dv[1].view(np.int32), h[1].view(np.int32))
    assert len(h[2]) == 3 and len(h[3]) == 3
    assert dv[2] == h[2] and dv[3] == h[3], (dv[2], h[2], dv[3], h[3])
    res, losses = dv[4]
    assert res is None
    assert losses.shape == (3 * 3,) and losses.dtype == np.float64 and np.all(np.isfinite(losses))
    # the first entry: the loss of the first mini-batch at the initial parameters, from the
    # float64 oracle; rtol as test_gpu_train.py holds train_'s losses to against that oracle
    data, chain, flow = _flow()
    np.testing.assert_array_equal(trainables(chain), p0)
    x_tr, th_tr = data.training_data()
    idx = np.random.default_rng(7).permutation(150)[:64]
    md = flow.metadata
    thn = O.normalize_input(th_tr[:, idx], md.theta_min, md.theta_max)
    ref = -float(np.mean(O.flow_logpdf(chain.to_spec(), x_tr[:, idx], thn, np.float64)))
    print("first step loss", losses[0], "oracle", ref)
    np.testing.assert_allclose(losses[0], ref, rtol=2e-4)


def test_train_debug_raises_alike_on_both_loaders(cuda, capsys):
    """Weights scaled until exp(s) overflows: the host loader's run is non-finite at its first
    step and raises ArgumentError; the device loader raises too and leaves the same parameters."""
    found = None
    for scale in (1e1, 1e2, 1e3, 1e4, 1e6):
        data, chain, flow = _flow(scale)
        state = setup(Adam(1e-3), flow)
        p0 = state.trainer.get_params().copy()
        capsys.readouterr()
        try:
            train_(flow, data, state, epochs=1, batchsize=64, verbose=False, debug=True,
                   rng=np.random.default_rng(7), loader="host")
        except _lib.ArgumentError:
            if np.array_equal(state.trainer.get_params().view(np.int32), p0.view(np.int32)):
                found = (scale, state.trainer.get_params(), trainables(chain))
                break
    assert found is not None, "no scale made the host loader's first step non-finite"
    scale, p_host, m_host = found
    host_out = capsys.readouterr().out
    data, chain, flow = _flow(scale)
    state = setup(Adam(1e-3), flow)
    with pytest.raises(_lib.ArgumentError, match="non-finite"):
        train_(flow, data, state, epochs=1, batchsize=64, verbose=False, debug=True,
               rng=np.random.default_rng(7), loader="device")
    assert state.trainer.steps_done == 0
    np.testing.assert_array_equal(state.trainer.get_params().view(np.int32), p_host.view(np.int32))
    np.testing.assert_array_equal(trainables(chain).view(np.int32), m_host.view(np.int32))
    dev_out = capsys.readouterr().out
    assert dev_out.strip() and dev_out == host_out          # the same batch's diagnostics
    assert flow.train_loss == [] and flow.valid_loss == []
