"""GPU tests of the optimiser chains (df_train_create_opt, df_train_adjust, df_train_grad_norms)
against the Float32 restatement in tests/opt_ref.py.

The optimiser is tested apart from the sweep: a crafted gradient is written into
``tr.grad()`` (which aliases the device buffer) and ``apply()`` runs the chain on it.  The
crafted vector has a tensor above ω, one below it, a zero tensor, entries beyond ±δ and
entries at exactly ±δ.

Criteria:
  * rules and chains: parameters within 1 ulp of opt_ref per step, the reference restarted
    from the device's parameters each step with its own m, v, βᵗ (as test_adam_step_and_repack);
    opt_ref's ClipNorm is fed the device's own norm (grad_norms() of the dx that reaches it);
  * grad_norms(): relative error <= (K + 3)·2⁻²⁴ against the float64 norm, K the longest
    chain of additions the kernel states (train.GRAD_NORM_K = kSumsqK): the summands are
    non-negative, so γ_K bounds the sum's error, the square root halves it, and one rounding
    per square and one for the root remain; bitwise reproducible;
  * a chain [Adam], graph replay, df_train_step_dist: bitwise.
"""
import ctypes as C
import os

import numpy as np
import pytest

import densityflows_amd as dfa
import densityflows_amd.train as train_mod
import opt_ref as R
from densityflows_amd import _lib
from densityflows_amd.train import (SWEEP_FUSED, SWEEP_LAYERWISE, Adam, AdamW, ClipGrad, ClipNorm, Descent, HIPTrainer,
                                    OptimiserChain, WeightDecay, adjust_, load_trainables, setup, train_, trainables)
from helpers import close, spec_to_element
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
DELTA, OMEGA = 0.05, 1.0


def _readme_spec(rng, hidden=16):
    """test/runtests.jl:103-109: three RNVP layers + NormalizationLayer; 2,322 parameters in
    tensors of 48, 16, 256, 16, 48 and 3 floats per conditioner."""
    layers = [O.rnvp_layer(rng, O.coupling_axes(5, m, n=1), hidden=hidden, bias_scale=0.1, out_scale=0.5)
              for m in ([1, 2, 3], [3, 4, 5], [5, 1, 2])]
    layers.append({"kind": "norm", "x_min": np.full(5, -3.0, np.float32), "x_max": np.full(5, 2.5, np.float32),
                   "alpha": -1.0, "beta": 1.0})
    return {"kind": "chain", "layers": layers}


def _wide_spec(rng):
    """The "wide" chain of test_gpu_train.py: 256 × 256 tensors (the largest the limits allow),
    a 3-Dense-hidden net at hidden 128; trains layer-wise."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(8, 4, n=3), hidden=256, bias_scale=0.1, out_scale=0.1),
        O.rnvp_layer(rng, O.coupling_axes(8, [2, 4, 6, 8, 1], n=3), n_sub=3, hidden=128, act="tanh",
                     bias_scale=0.1, out_scale=0.2),
        {"kind": "norm", "x_min": np.full(8, -3.0, np.float32), "x_max": np.full(8, 3.5, np.float32),
         "alpha": 0.0, "beta": 1.0},
    ]}


SPECS = {"readme": (_readme_spec, 5, 1), "wide": (_wide_spec, 8, 3)}
# (chain, requested sweep): the fused sweep where the chain takes it, the layer-wise one everywhere
PATHS = [("readme", SWEEP_FUSED), ("readme", SWEEP_LAYERWISE), ("wide", SWEEP_LAYERWISE)]
PATH_IDS = ["readme-fused", "readme-layerwise", "wide-layerwise"]
README_PATHS = PATHS[:2]


def _setup(name, seed=0):
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(seed))
    return spec, spec_to_element(spec), d, n


def _trainer(spec, opt, sweep):
    chain = spec_to_element(spec)           # a trainer repacks its chain's weights: one chain each
    tr = HIPTrainer(chain.hip(), opt, sweep)
    assert (tr.sweep() == SWEEP_FUSED) == (sweep == SWEEP_FUSED)
    return chain, tr


def _inputs(d, n, B, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d, B)).astype(np.float32)
    th = rng.random((n, B)).astype(np.float32) if n > 0 else np.zeros((0, B), np.float32)
    return x, th


def _dev(a, dev):
    """numpy (rows, B) → flat Julia-order device buffer."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T).ravel()).to(dev)


def _ulp_diff(a, b):
    ai = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    bi = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.max(np.abs(ai - bi))) if ai.size else 0


def _crafted(offs, seed):
    """A gradient with per-tensor norms 3ω, ω/2, 0, then 2ω and ω/4 alternating, and in the
    fourth tensor entries at exactly ±δ and beyond ±δ."""
    rng = np.random.default_rng(seed)
    g = np.zeros(offs[-1], F)
    scale = [3.0, 0.5, 0.0]
    for k, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        s = scale[k] if k < 3 else (2.0 if k % 2 else 0.25)
        v = rng.standard_normal(b - a)
        g[a:b] = (v * (s * OMEGA / np.sqrt(np.sum(v * v)))).astype(F)
    a = offs[3]
    assert offs[4] - a >= 6
    g[a:a + 6] = np.array([DELTA, -DELTA, 3 * DELTA, -4 * DELTA, DELTA / 2, -DELTA / 3], F)
    n = R.norms64(g, offs)
    assert n[0] > 2 * OMEGA and 0 < n[1] < 0.6 * OMEGA and n[2] == 0.0
    assert np.any(np.abs(g) > F(DELTA)) and np.any(g == F(DELTA)) and np.any(g == -F(DELTA))
    return g


def _set_grad(tr, g):
    import torch

    tr.grad().copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=F)))


def _device_norms(tr, x, g, opt):
    """The device's own norm of the dx that reaches the chain's ClipNorm: grad_norms() of that
    dx (rounded op for op as the kernel rounds it), the gradient then put back."""
    import torch

    pre = R.pre_clip_dx(x, g, opt)
    if pre is None:
        return None
    _set_grad(tr, pre)
    nd = tr.grad_norms()
    torch.cuda.synchronize()
    _set_grad(tr, g)
    return nd.cpu().numpy()


def _apply_and_check(tr, opt, st, offs, g):
    """One injected-gradient step on the device against opt_ref from the device's parameters."""
    import torch

    p = tr.get_params().copy()
    nd = _device_norms(tr, p, g, opt)
    _set_grad(tr, g)
    tr.apply()
    torch.cuda.synchronize()
    want, _ = R.chain_update(p, g, opt, st, offs, norms=nd)
    got = tr.get_params()
    assert _ulp_diff(got, want) <= 1, (repr(opt), _ulp_diff(got, want))
    return p, got


# ---- 1. the existing path ------------------------------------------------------------

@pytest.mark.parametrize("name,sweep", PATHS, ids=PATH_IDS)
def test_chain_of_adam_is_the_plain_adam_trainer(cuda, name, sweep):
    """df_train_create_opt with [Adam] leaves bitwise the parameters of a df_train_create_ex
    trainer over three steps."""
    import torch

    spec, _, d, n = _setup(name)
    _, plain = _trainer(spec, Adam(2e-3, (0.8, 0.99), 1e-7), sweep)
    _, chained = _trainer(spec, OptimiserChain(Adam(2e-3, (0.8, 0.99), 1e-7)), sweep)
    for step in range(3):
        x, th = _inputs(d, n, 300, seed=20 + step)
        xd, td = _dev(x, cuda), (_dev(th, cuda) if n else None)
        plain.step(xd, td, 300)
        chained.step(xd, td, 300)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(chained.get_params(), plain.get_params())
    assert not np.array_equal(plain.get_params(), trainables(spec_to_element(spec)))


# ---- 2. grad_norms ----------------------------------------------------------------------

@pytest.mark.parametrize("name,sweep", PATHS, ids=PATH_IDS)
def test_grad_norms_against_float64(cuda, name, sweep):
    import torch

    spec, _, d, n = _setup(name)
    _, tr = _trainer(spec, Adam(), sweep)
    offs = tr.tensor_offsets()
    assert offs[0] == 0 and offs[-1] == tr.num_params and np.all(np.diff(offs) > 0)
    if name == "readme":
        assert list(np.diff(offs)) == [48, 16, 256, 16, 48, 3] * 6
    else:
        assert np.max(np.diff(offs)) == 256 * 256
    rng = np.random.default_rng(5)
    g = (rng.standard_normal(offs[-1]) * np.exp(rng.uniform(-6, 2, offs[-1]))).astype(F)
    g[offs[2]:offs[3]] = 0.0
    _set_grad(tr, g)
    got = tr.grad_norms()
    again = tr.grad_norms()
    torch.cuda.synchronize()
    got, again = got.cpu().numpy(), again.cpu().numpy()
    want = R.norms64(g, offs)
    assert got.dtype == F and got.shape == (offs.shape[0] - 1,)
    rel = np.abs(got.astype(np.float64) - want) / np.where(want > 0, want, 1.0)
    bound = (train_mod.GRAD_NORM_K + 3) * 2.0 ** -24
    print("grad_norms max relative error", rel.max(), "bound", bound)
    assert got[2] == 0.0
    assert np.all(rel <= bound), (rel.max(), bound)
    assert got.tobytes() == again.tobytes()
    np.testing.assert_array_equal(tr.grad().cpu().numpy(), g)       # changes no state
    _, tr2 = _trainer(spec, OptimiserChain(ClipNorm(1.0), Adam()), sweep)
    _set_grad(tr2, g)
    other = tr2.grad_norms()
    torch.cuda.synchronize()
    assert other.cpu().numpy().tobytes() == got.tobytes()


# ---- 3. every rule and the chains against opt_ref -----------------------------------------

A = lambda: Adam(2e-3, (0.8, 0.99), 1e-7)
CHAINS = {
    "clipgrad-adam": lambda: OptimiserChain(ClipGrad(DELTA), A()),
    "clipnorm-adam": lambda: OptimiserChain(ClipNorm(OMEGA), A()),
    "decay-adam": lambda: OptimiserChain(WeightDecay(0.02), A()),
    "descent-adam": lambda: OptimiserChain(Descent(0.5), A()),
    "adamw": lambda: AdamW(2e-3, (0.8, 0.99), 0.01, 1e-7),
    "clipgrad-decay-adam": lambda: OptimiserChain(ClipGrad(DELTA), WeightDecay(0.02), A()),
    "decay-clipgrad-adam": lambda: OptimiserChain(WeightDecay(0.02), ClipGrad(DELTA), A()),
    "decay-clipnorm-adam": lambda: OptimiserChain(WeightDecay(0.5), ClipNorm(OMEGA), A()),
    "clipnorm-adam-decay": lambda: OptimiserChain(ClipNorm(OMEGA), A(), WeightDecay(0.01)),
    "clipnorm-descent": lambda: OptimiserChain(ClipNorm(OMEGA), Descent(0.01)),
}


@pytest.mark.parametrize("which", list(CHAINS))
@pytest.mark.parametrize("name,sweep", PATHS, ids=PATH_IDS)
def test_chain_steps_match_opt_ref(cuda, name, sweep, which):
    """Two injected-gradient steps (βᵗ advances) within 1 ulp of opt_ref, then the chain's
    packed weights follow the update: backward on the device matches the oracle on the new
    parameters."""
    spec, _, d, n = _setup(name)
    opt = CHAINS[which]()
    chain, tr = _trainer(spec, opt, sweep)
    offs = tr.tensor_offsets()
    st = R.new_state(tr.num_params, opt)
    p0 = tr.get_params().copy()
    for step in range(2):
        _apply_and_check(tr, opt, st, offs, _crafted(offs, 40 + step))
    assert not np.array_equal(tr.get_params(), p0)
    load_trainables(chain, tr.get_params())
    x, th = _inputs(d, n, 300, seed=99)
    z, l = dfa.backward(chain, x, th if n else None)
    zo, lo = O.backward(chain.to_spec(), x, th if n else np.zeros((0, 300)))
    assert close(z, zo)[0] and close(l, lo)[0]


@pytest.mark.parametrize("name,sweep", PATHS, ids=PATH_IDS)
def test_unclipped_dx_is_bitwise_untouched(cuda, name, sweep):
    """[ClipNorm, Descent(1)]: tensors at or below ω (the zero tensor too) get x_new = x - g
    exactly, the others x - g·(ω / nrm); [ClipGrad, Descent(1)]: entries within ±δ get
    x - g exactly, the others x ∓ δ."""
    import torch

    spec, _, d, n = _setup(name)
    opt = OptimiserChain(ClipNorm(OMEGA), Descent(1.0))
    _, tr = _trainer(spec, opt, sweep)
    offs = tr.tensor_offsets()
    g = _crafted(offs, 7)
    p, got = _apply_and_check(tr, opt, R.new_state(tr.num_params, opt), offs, g)
    below = above = 0
    nrm = R.norms64(g, offs)
    for k, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        if nrm[k] < 0.9 * OMEGA:
            assert got[a:b].tobytes() == (p[a:b] - g[a:b]).tobytes(), k
            below += 1
        elif nrm[k] > 1.1 * OMEGA:
            assert not np.array_equal(got[a:b], p[a:b] - g[a:b]), k
            above += 1
    assert below >= 2 and above >= 2
    opt = OptimiserChain(ClipGrad(DELTA), Descent(1.0))
    _, tr = _trainer(spec, opt, sweep)
    p = tr.get_params().copy()
    _set_grad(tr, g)
    tr.apply()
    torch.cuda.synchronize()
    got = tr.get_params()
    inside = np.abs(g) <= F(DELTA)
    assert 0 < np.count_nonzero(~inside) < g.size
    assert got[inside].tobytes() == (p - g)[inside].tobytes()
    assert got[~inside].tobytes() == (p - np.sign(g) * F(DELTA))[~inside].astype(F).tobytes()


# ---- 4. adjust -------------------------------------------------------------------------

ADJ = {"adam": lambda eta: Adam(eta, (0.8, 0.99), 1e-7),
       "clipnorm-adam-decay": lambda eta: OptimiserChain(ClipNorm(OMEGA), Adam(eta, (0.8, 0.99), 1e-7), WeightDecay(0.01)),
       "clipgrad-descent": lambda eta: OptimiserChain(ClipGrad(DELTA), Descent(eta))}


@pytest.mark.parametrize("which", list(ADJ))
@pytest.mark.parametrize("name,sweep", README_PATHS, ids=PATH_IDS[:2])
def test_adjust_keeps_the_moments(cuda, name, sweep, which):
    """Three steps at η₁, adjust(η₂), three steps: opt_ref with m, v, βᵗ carried across.  A
    fresh trainer at η₂ started from the parameters at the adjust ends elsewhere (its moments
    start at zero) unless the chain has no state."""
    import torch

    eta1, eta2 = 2e-3, 5e-4
    spec, _, d, n = _setup(name)
    _, tr = _trainer(spec, ADJ[which](eta1), sweep)
    offs = tr.tensor_offsets()
    st = R.new_state(tr.num_params, ADJ[which](eta1))
    for step in range(3):
        _apply_and_check(tr, ADJ[which](eta1), st, offs, _crafted(offs, 60 + step))
    tr.adjust(eta2)
    mid = tr.get_params().copy()
    for step in range(3, 6):
        _apply_and_check(tr, ADJ[which](eta2), st, offs, _crafted(offs, 60 + step))
    _, fresh = _trainer(spec, ADJ[which](eta2), sweep)
    fresh.set_params(mid)
    for step in range(3, 6):
        _set_grad(fresh, _crafted(offs, 60 + step))
        fresh.apply()
    torch.cuda.synchronize()
    assert np.array_equal(fresh.get_params(), tr.get_params()) == (which == "clipgrad-descent")
    with pytest.raises(_lib.ArgumentError):
        tr.adjust(-1.0)


@pytest.mark.parametrize("which", list(ADJ))
@pytest.mark.parametrize("name,sweep", README_PATHS, ids=PATH_IDS[:2])
def test_adjust_recaptures_the_graph(cuda, name, sweep, which):
    """step_graph through an adjust equals the eager sequence bit for bit: eager, capture and
    two replays at η₁ (so a graph captured with η₁ exists when η changes), then the same at η₂."""
    import torch

    spec, _, d, n = _setup(name)
    _, eager = _trainer(spec, ADJ[which](2e-3), sweep)
    _, graph = _trainer(spec, ADJ[which](2e-3), sweep)
    _, stale = _trainer(spec, ADJ[which](2e-3), sweep)     # never adjusted: what a stale replay would give
    x, th = _inputs(d, n, 64, seed=3)
    xd, td = _dev(x, cuda), _dev(th, cuda)
    xs, ts = xd.clone(), td.clone()
    for i in range(8):
        if i == 4:
            eager.adjust(5e-4)
            graph.adjust(5e-4)
        eager.step(xd, td, 64)
        graph.step_graph(xs, ts, 64)
        stale.step(xd, td, 64)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(graph.get_params(), eager.get_params(), err_msg=f"step {i}")
        assert np.array_equal(stale.get_params(), eager.get_params()) == (i < 4)


# ---- 5. graph equals eager --------------------------------------------------------------

def _median_norm(spec, d, n, B, cuda, sweep):
    """A ClipNorm bound some tensors of the first gradient exceed and some do not."""
    import torch

    _, probe = _trainer(spec, Adam(), sweep)
    x, th = _inputs(d, n, B, seed=B)
    probe.gradient(_dev(x, cuda), _dev(th, cuda), B, B)
    nrm = probe.grad_norms()
    torch.cuda.synchronize()
    nrm = nrm.cpu().numpy()
    omega = float(np.median(nrm))
    assert np.count_nonzero(nrm > 1.05 * omega) >= 2 and np.count_nonzero(nrm < 0.95 * omega) >= 2
    return omega


@pytest.mark.parametrize("name,sweep", PATHS, ids=PATH_IDS)
def test_step_graph_equals_eager_with_a_chain(cuda, name, sweep):
    import torch

    spec, _, d, n = _setup(name, seed=7)
    omega = _median_norm(spec, d, n, 64, cuda, sweep)
    opt = lambda: OptimiserChain(ClipNorm(omega), Adam(1e-3), WeightDecay(1e-3))
    _, eager = _trainer(spec, opt(), sweep)
    _, graph = _trainer(spec, opt(), sweep)
    x, th = _inputs(d, n, 64, seed=64)
    xd, td = _dev(x, cuda), _dev(th, cuda)
    xs, ts = xd.clone(), td.clone()
    for i in range(8):
        eager.step(xd, td, 64)
        graph.step_graph(xs, ts, 64)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(graph.get_params(), eager.get_params(), err_msg=f"step {i}")


# ---- 6. df_train_step_dist ----------------------------------------------------------------

@pytest.mark.parametrize("name,sweep", README_PATHS, ids=PATH_IDS[:2])
def test_world1_step_dist_with_a_chain_equals_local_step(cuda, name, sweep):
    """The chain runs inside df_train_apply, after the all-reduce: through a world-1 RCCL
    communicator the step is bitwise the local one."""
    import torch

    from densityflows_amd.parallel import DFComm

    try:
        comm = DFComm(0)
    except _lib.UnsupportedError as e:           # no RCCL on this machine
        pytest.skip(str(e))
    try:
        spec, _, d, n = _setup(name, seed=2)
        omega = _median_norm(spec, d, n, 512, cuda, sweep)
        x, th = _inputs(d, n, 512, seed=512)
        xd, td = _dev(x, cuda), _dev(th, cuda)
        out = []
        for dist_step in (False, True):
            _, tr = _trainer(spec, OptimiserChain(ClipNorm(omega), Adam(1e-3), WeightDecay(1e-3)), sweep)
            for _ in range(3):
                if dist_step:
                    tr.step_dist(comm, xd, td, 512, 512)
                else:
                    tr.step(xd, td, 512)
            torch.cuda.synchronize()
            out.append(tr.get_params())
        np.testing.assert_array_equal(out[0], out[1])
    finally:
        comm.close()


# ---- 7. train_ -------------------------------------------------------------------------

def _datatest_flow(seed=0):
    here = os.path.join(os.path.dirname(__file__), "golden")
    x = np.load(os.path.join(here, "datatest_x.npy"))
    th = np.load(os.path.join(here, "datatest_theta.npy"))
    rng = np.random.default_rng(seed)
    data = dfa.DataArrays(x, th, rng=rng)
    chain = dfa.FlowChain(
        dfa.CouplingLayer(data, [1, 2, 3], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.CouplingLayer(data, [3, 4, 5], hidden_dim_s=16, hidden_dim_t=16, σ="tanh", rng=rng),
        dfa.CouplingLayer(data, [5, 1, 2], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.NormalizationLayer.from_data(x, -1.0, 1.0))
    return data, chain, dfa.Flow(chain, data)


def _flat_oracle_grads(spec, grads):
    parts = []
    for L, g in zip(O._flat_layers(spec), grads):
        if L["kind"] == "norm":
            continue
        for net in ("s_net", "t_net"):
            if net not in L:
                continue
            for (dW, db), D in zip(g[net], L[net]):
                parts.append(np.asarray(dW).ravel(order="F"))
                if D.get("b") is not None:
                    parts.append(np.asarray(db))
    return np.concatenate(parts)


@pytest.mark.parametrize("sweep", [SWEEP_FUSED, SWEEP_LAYERWISE], ids=["fused", "layerwise"])
def test_train_epochs_with_clipnorm_match_oracle_loop(cuda, monkeypatch, sweep):
    """Two epochs of train_ (shuffle off, batchsize 64) with OptimiserChain(ClipNorm(ω), Adam())
    against the oracle-gradient + opt_ref loop: the pushed losses agree to the tolerance of
    test_train_epochs_match_oracle_loop.  ω = 0.75 sits inside the spread of the first
    gradients' tensor norms (0.31 .. 1.47 on the CPU oracle), so some tensors clip and some
    do not; asserted below on the oracle's gradients."""
    monkeypatch.setattr(train_mod, "DEFAULT_SWEEP", sweep)
    omega = 0.75
    opt = OptimiserChain(ClipNorm(omega), Adam(1e-3))
    data, chain, flow = _datatest_flow(seed=3)
    spec0 = chain.to_spec()
    state = setup(opt, flow)
    offs = state.trainer.tensor_offsets()
    assert (state.trainer.sweep() == SWEEP_FUSED) == (sweep == SWEEP_FUSED)
    train_(flow, data, state, epochs=2, batchsize=64, shuffle=False, verbose=False, graphs=True)
    md = flow.metadata
    x_tr, th_tr = data.training_data()
    x_va, th_va = data.validation_data()
    thn_tr = O.normalize_input(th_tr, md.theta_min, md.theta_max)
    thn_va = O.normalize_input(th_va, md.theta_min, md.theta_max)
    _, chain_o, _ = _datatest_flow(seed=3)
    p = trainables(chain_o).astype(np.float32)
    st = R.new_state(p.shape[0], opt)
    spec = spec0
    tl, vl = [], []
    N = x_tr.shape[1]
    clipped = kept = 0
    for ep in range(2):
        for b0 in range(0, N, 64):
            _, g = O.nll_and_grad(spec, x_tr[:, b0:b0 + 64], thn_tr[:, b0:b0 + 64])
            g = _flat_oracle_grads(spec, g).astype(np.float32)
            if ep == 0 and b0 < 3 * 64:
                nrm = R.norms64(g, offs)
                clipped += int(np.count_nonzero(nrm > 1.05 * omega))
                kept += int(np.count_nonzero(nrm < 0.95 * omega))
            p, _ = R.chain_update(p, g, opt, st, offs)
            load_trainables(chain_o, p)
            spec = chain_o.to_spec()
        tl.append(-float(np.mean(O.flow_logpdf(spec, x_tr, thn_tr, np.float64))))
        vl.append(-float(np.mean(O.flow_logpdf(spec, x_va, thn_va, np.float64))))
    assert clipped >= 6 and kept >= 6, (clipped, kept)
    print("train_loss", flow.train_loss, tl, "valid_loss", flow.valid_loss, vl)
    np.testing.assert_allclose(flow.train_loss, tl, rtol=2e-4)
    np.testing.assert_allclose(flow.valid_loss, vl, rtol=2e-4)
    adjust_(state, 5e-4)                         # Optimisers.adjust! on a TrainState
    train_(flow, data, state, epochs=1, batchsize=64, shuffle=False, verbose=False)
    assert len(flow.train_loss) == 3 and np.isfinite(flow.train_loss[-1])


# ---- 8. refusals -----------------------------------------------------------------------

def _rules(*kp):
    return (_lib.df_opt_rule * len(kp))(*[_lib.df_opt_rule(k, tuple(p) + (0.0,) * (4 - len(p))) for k, p in kp])


_ADAM = (_lib.DF_OPT_ADAM, (1e-3, 0.9, 0.999, 1e-8))
REFUSED = {
    "two-adam": ([_ADAM, _ADAM], _lib.DF_ERR_UNSUPPORTED, "Adam",
                 lambda: OptimiserChain(Adam(), Adam())),
    "two-clipnorm": ([(_lib.DF_OPT_CLIP_NORM, (1.0,)), (_lib.DF_OPT_CLIP_NORM, (2.0,)), _ADAM],
                     _lib.DF_ERR_UNSUPPORTED, "ClipNorm", lambda: OptimiserChain(ClipNorm(1.0), ClipNorm(2.0), Adam())),
    "no-terminal": ([(_lib.DF_OPT_CLIP_GRAD, (1.0,)), (_lib.DF_OPT_WEIGHT_DECAY, (0.1,))],
                    _lib.DF_ERR_UNSUPPORTED, "terminal", lambda: OptimiserChain(ClipGrad(1.0), WeightDecay(0.1))),
    "nine-rules": ([(_lib.DF_OPT_CLIP_GRAD, (1.0,))] * 8 + [_ADAM], _lib.DF_ERR_UNSUPPORTED, "8 rules",
                   lambda: OptimiserChain(*([ClipGrad(1.0)] * 8), Adam())),
    "delta-zero": ([(_lib.DF_OPT_CLIP_GRAD, (0.0,)), _ADAM], _lib.DF_ERR_INVALID, "ClipGrad",
                   lambda: OptimiserChain(ClipGrad(0.0), Adam())),
    "omega-nan": ([(_lib.DF_OPT_CLIP_NORM, (float("nan"),)), _ADAM], _lib.DF_ERR_INVALID, "ClipNorm",
                  lambda: OptimiserChain(ClipNorm(float("nan")), Adam())),
    "lambda-negative": ([(_lib.DF_OPT_WEIGHT_DECAY, (-0.1,)), _ADAM], _lib.DF_ERR_INVALID, "WeightDecay",
                        lambda: OptimiserChain(WeightDecay(-0.1), Adam())),
    "clipnorm-after-adam": ([_ADAM, (_lib.DF_OPT_CLIP_NORM, (1.0,))], _lib.DF_ERR_UNSUPPORTED, "ClipNorm",
                            lambda: OptimiserChain(Adam(), ClipNorm(1.0))),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_chains_leave_the_chain_usable(cuda, case):
    """The library refuses what the Python classes refuse, with the documented status and a
    message that names the rule; a trainer created afterwards on the same chain works."""
    import torch

    rules, status, word, make = REFUSED[case]
    spec, chain, d, n = _setup("readme")
    hc = chain.hip()
    h = C.c_void_p()
    arr = _rules(*rules)
    rc = hc.lib.df_train_create_opt(C.byref(h), hc.handle, arr, len(rules), 0)
    assert rc == status and not h.value
    assert word in hc.lib.df_last_error().decode()
    with pytest.raises(_lib.UnsupportedError if status == _lib.DF_ERR_UNSUPPORTED else _lib.ArgumentError, match=word):
        HIPTrainer(hc, make())
    tr = HIPTrainer(hc, OptimiserChain(ClipGrad(1.0), ClipNorm(1.0), Adam()))
    p0 = tr.get_params().copy()
    x, th = _inputs(d, n, 64)
    tr.step(_dev(x, cuda), _dev(th, cuda), 64)
    torch.cuda.synchronize()
    p1 = tr.get_params()
    assert np.all(np.isfinite(p1)) and not np.array_equal(p1, p0)
