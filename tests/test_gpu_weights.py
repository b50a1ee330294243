"""Sample weights on the GPU: the weighted loss  -Σ w·logpdf / Σ w, its gradient, the captured
and epoch forms of its step, and train_ on DataArrays(weights=).

References: tests/weights_ref.py (the fp64 oracle on the duplicated batch for integer
weights, Σ w_i·g_i / W per sample for real ones) and the GPU's own unweighted calls (unit
weights and the duplicated batch).  Chains, inputs, cases and the gradient criterion are
tests/train_edge_cases.py's; as in tests/test_gpu_train_edges.py the grids are sized from
DF_GRID_CUS=2, so the largest batches pass one trip of every batch loop.
"""
import ctypes as C

import numpy as np
import pytest

import densityflows_amd as dfa
import densityflows_amd.train as train_mod
import test_gpu_train_edges as E
import train_edge_cases as T
import weights_ref as WR
from densityflows_amd import _lib
from densityflows_amd.train import Adam, HIPTrainer, load_trainables, setup, train_, trainables, weighted_nll
from helpers import close, spec_to_element
from train_edge_cases import CASES, G_ATOL, G_RTOL, _tensor_slices, largest_batches

pytestmark = pytest.mark.gpu

PARITY_CASES = ("readme", "cfg2", "pre", "mixed", "readme_lw", "wide_kept", "cfg5x2_h0free")
# one past one span of the fp64 reductions (kWsumSpan = 16 · 256 elements per workgroup,
# csrc/df_train.h): two workgroups and the second launch that adds their sums
WSUM_SPAN = 4096


def _dev(a, dev):
    import torch

    a = np.asarray(a, np.float32)
    if a.shape[0] == 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)


def _wdev(w, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev)


def _sums(dev, n=2):
    import torch

    return torch.zeros(n, dtype=torch.float64, device=dev)


def _wgrad(tr, x, th, w, dev, w_total=0.0):
    """Weighted gradient of the batch (x, θ, w) → (flat gradient, wsums)."""
    import torch

    ws = _sums(dev)
    tr.gradient(_dev(x, dev), _dev(th, dev), x.shape[1], w=_wdev(w, dev), w_total=w_total, wsums=ws)
    torch.cuda.synchronize()
    return tr.grad().detach().cpu().numpy().copy(), ws.cpu().numpy()


def _ugrad(tr, x, th, dev):
    import torch

    lp = _sums(dev, 1)
    tr.gradient(_dev(x, dev), _dev(th, dev), x.shape[1], x.shape[1], lp)
    torch.cuda.synchronize()
    return tr.grad().detach().cpu().numpy().copy(), float(lp.item())


def _worst(spec, g, ref):
    assert g.shape == ref.shape and np.all(np.isfinite(g))
    return max(close(g[sl], ref[sl], G_RTOL, G_ATOL)[1] for sl in _tensor_slices(spec))


def _ints(B):
    if B == 1:
        return np.array([2])
    k = np.random.default_rng(11).choice([0, 1, 2], size=B, p=[.25, .5, .25])
    assert k.sum() > 0
    return k


def _plain_trainer(chain, sweep="AUTO"):
    spec = T.case_data(chain)[0]
    return spec, HIPTrainer(spec_to_element(spec).hip(), Adam(), sweep=getattr(train_mod, "SWEEP_" + sweep))


# ---- 1. parity matrix ---------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("case", PARITY_CASES)
def test_integer_weights_match_the_duplicated_batch(cuda, case, which, monkeypatch, capfd):
    chain, sweep, form, env = CASES[case]
    spec, d, n, x, th = T.case_data(chain)
    B = (1, 17, largest_batches(form)[-1])[which]
    tr, info = E._trainer(chain, sweep, env, T.GRID_CUS, monkeypatch, capfd)
    E._check_grids(info, T.GRID_CUS, form, case)
    k = _ints(B)
    xb, tb = x[:, :B], th[:, :B]
    g, ws = _wgrad(tr, xb, tb, k, cuda)
    assert tr.sweep() == getattr(train_mod, "SWEEP_" + form), f"{case}: sweep form {tr.sweep()}"
    assert ws[1] == float(k.sum()), f"{case} B={B}: W = {ws[1]!r}, Σk = {k.sum()}"
    # the GPU's unweighted gradient of the duplicated batch: the same per-sample f32
    # arithmetic, only the order of the sums differs
    xd, td = WR.duplicated(xb, tb, k)
    gd, lpd = _ugrad(tr, xd, td, cuda)
    r_dup = _worst(spec, g, gd)
    loss, ref = WR.integer_weight_grad(spec, xb, tb, k)
    r_ref = _worst(spec, g, ref)
    got = -ws[0] / ws[1]
    capfd.readouterr()
    print(f"WEIGHTS {case} B={B} Σk={k.sum()}: ratio oracle {r_ref:.3f} duplicated {r_dup:.3f} "
          f"loss {got} oracle {loss} duplicated {-lpd / k.sum()}")
    assert abs(got - loss) <= 1e-5 * max(1.0, abs(loss)), f"{case} B={B}: loss {got} against {loss}"
    assert r_dup <= 1.0, f"{case} B={B}: violation ratio {r_dup} against the GPU's duplicated batch"
    assert r_ref <= 1.0, f"{case} B={B}: violation ratio {r_ref} against the oracle"


# ---- 2. unit weights ----------------------------------------------------------------------

@pytest.mark.parametrize("case", ["readme", "cfg2", "wide_kept"])
def test_unit_weights_are_the_unweighted_step_bitwise(cuda, case, monkeypatch, capfd):
    import torch

    chain, sweep, form, env = CASES[case]
    spec, d, n, x, th = T.case_data(chain)
    B = 777
    xb, tb, w = _dev(x[:, :B], cuda), _dev(th[:, :B], cuda), _wdev(np.ones(B), cuda)
    a, _ = E._trainer(chain, sweep, env, T.GRID_CUS, monkeypatch, capfd)
    b, _ = E._trainer(chain, sweep, env, T.GRID_CUS, monkeypatch, capfd)
    ws, lp = _sums(cuda), _sums(cuda, 1)
    a.gradient(xb, tb, B, w=w, wsums=ws)
    b.gradient(xb, tb, B, B, lp)
    torch.cuda.synchronize()
    assert E._same_bits(a.grad().cpu().numpy(), b.grad().cpu().numpy()), f"{case}: gradients differ"
    ws_h, lp_h = ws.cpu().numpy(), float(lp.item())
    print(f"WEIGHTS unit {case}: Σ w·lp {ws_h[0]!r} Σ lp {lp_h!r} W {ws_h[1]!r}")
    assert ws_h[1] == float(B)
    assert abs(ws_h[0] - lp_h) <= 1e-12 * abs(lp_h), f"{case}: Σ w·lp {ws_h[0]!r} against Σ logpdf {lp_h!r}"
    a.step(xb, tb, B, w=w)
    b.step(xb, tb, B)
    torch.cuda.synchronize()
    assert E._same_bits(a.get_params(), b.get_params()), f"{case}: parameters after one step differ"


# ---- 3. scale invariance ------------------------------------------------------------------

def test_scaling_the_weights(cuda):
    spec, tr = _plain_trainer("readme")
    _, d, n, x, th = T.case_data("readme")
    B = 333
    w = (np.random.default_rng(3).random(B) + 0.1).astype(np.float32)
    g, ws = _wgrad(tr, x[:, :B], th[:, :B], w, cuda)
    g4, ws4 = _wgrad(tr, x[:, :B], th[:, :B], np.float32(0.25) * w, cuda)
    assert E._same_bits(g, g4), "0.25·w changed the gradient"
    assert ws4[1] == 0.25 * ws[1] and ws4[0] == 0.25 * ws[0]
    g37, ws37 = _wgrad(tr, x[:, :B], th[:, :B], np.float32(0.37) * w, cuda)
    r = _worst(spec, g37, g)
    print(f"WEIGHTS scale 0.37: ratio {r:.4f}")
    assert r <= 1.0
    assert abs(ws37[0] / ws37[1] - ws[0] / ws[1]) <= 1e-5 * max(1.0, abs(ws[0] / ws[1]))


# ---- 4. real weights ----------------------------------------------------------------------

@pytest.mark.parametrize("chain", ["readme", "mixed"])
def test_real_weights_match_the_per_sample_reference(cuda, chain):
    spec, tr = _plain_trainer(chain)
    _, d, n, x, th = T.case_data(chain)
    B = 37
    w = (np.random.default_rng(3).random(B) + 0.1).astype(np.float32)
    g, ws = _wgrad(tr, x[:, :B], th[:, :B], w, cuda)
    loss, ref = WR.per_sample_grad(spec, x[:, :B], th[:, :B], w)
    r = _worst(spec, g, ref)
    print(f"WEIGHTS real {chain}: ratio {r:.3f} loss {-ws[0] / ws[1]} oracle {loss}")
    assert abs(ws[1] - float(np.sum(w, dtype=np.float64))) <= 1e-12 * ws[1]
    assert abs(-ws[0] / ws[1] - loss) <= 1e-5 * max(1.0, abs(loss))
    assert r <= 1.0


# ---- 5. zero weights and guards -----------------------------------------------------------

def test_zero_weight_samples_and_the_rows_past_the_batch(cuda):
    import torch

    spec, tr = _plain_trainer("readme")
    _, d, n, x, th = T.case_data("readme")
    B, extra = 200, 77
    w = (np.random.default_rng(3).random(B) + 0.1).astype(np.float32)
    g, ws = _wgrad(tr, x[:, :B], th[:, :B], w, cuda)
    # zero-weight finite samples appended: the same gradient at the criterion (the tiles and
    # the workgroups' shares move, the sums do not gain a term)
    wz = np.concatenate([w, np.zeros(extra, np.float32)])
    gz, wsz = _wgrad(tr, x[:, :B + extra], th[:, :B + extra], wz, cuda)
    r = _worst(spec, gz, g)
    print(f"WEIGHTS zero-weight tail: ratio {r:.4f}")
    assert r <= 1.0 and wsz[1] == ws[1]
    assert abs(wsz[0] - ws[0]) <= 1e-12 * abs(ws[0])
    # NaN in x, θ and w past `batch`: nothing of it is read
    pad = 2 * 512 + 7
    xb, tb = E._poisoned(x, B, pad, cuda), E._poisoned(th, B, pad, cuda)
    wb = torch.full((B + pad,), float("nan"), dtype=torch.float32, device=cuda)
    wb[:B] = _wdev(w, cuda)
    ws2 = _sums(cuda)
    tr.gradient(xb, tb, B, w=wb, wsums=ws2)
    torch.cuda.synchronize()
    assert E._same_bits(tr.grad().cpu().numpy(), g)
    assert np.array_equal(ws2.cpu().numpy().view(np.int64), ws.view(np.int64))


# ---- 6. shards ----------------------------------------------------------------------------

def test_shards_with_the_global_weight_sum_add_up(cuda):
    spec, tr = _plain_trainer("readme")
    _, d, n, x, th = T.case_data("readme")
    B, cut = 333, 101
    w = (np.random.default_rng(3).random(B) + 0.1).astype(np.float32)
    g, ws = _wgrad(tr, x[:, :B], th[:, :B], w, cuda)
    W = float(ws[1])
    ga, wa = _wgrad(tr, x[:, :cut], th[:, :cut], w[:cut], cuda, w_total=W)
    gb, wb = _wgrad(tr, x[:, cut:B], th[:, cut:B], w[cut:], cuda, w_total=W)
    assert wa[1] == W and wb[1] == W
    assert abs(wa[0] + wb[0] - ws[0]) <= 1e-12 * abs(ws[0])
    r = _worst(spec, ga + gb, g)
    print(f"WEIGHTS shards: ratio {r:.4f}")
    assert r <= 1.0


# ---- 7. captured step ---------------------------------------------------------------------

def test_captured_weighted_step_equals_the_eager_loop(cuda):
    import torch

    _, d, n, x, th = T.case_data("readme")
    _, a = _plain_trainer("readme")
    _, b = _plain_trainer("readme")
    B = 64
    rng = np.random.default_rng(5)
    xb = torch.empty(B * d, dtype=torch.float32, device=cuda)
    tb = torch.empty(B * n, dtype=torch.float32, device=cuda)
    wb = torch.empty(B, dtype=torch.float32, device=cuda)
    ws = _sums(cuda)
    for i in range(4):
        idx = rng.permutation(T.B_LIMIT)[:B]
        w = (rng.random(B) * (i + 1) + 0.1).astype(np.float32)    # (another Σ w at every call)
        xb.copy_(_dev(x[:, idx], cuda))
        tb.copy_(_dev(th[:, idx], cuda))
        wb.copy_(_wdev(w, cuda))
        a.step_graph(xb, tb, B, w=wb, wsums=ws)
        ws_e = _sums(cuda)
        b.step(_dev(x[:, idx], cuda), _dev(th[:, idx], cuda), B, w=_wdev(w, cuda), wsums=ws_e)
        torch.cuda.synchronize()
        assert np.array_equal(ws.cpu().numpy().view(np.int64), ws_e.cpu().numpy().view(np.int64)), f"call {i}"
        assert E._same_bits(a.get_params(), b.get_params()), f"call {i}: parameters differ"


# ---- 8. epochs ----------------------------------------------------------------------------

def _hand_epoch(tr, xs, ts, wt, N, d, n, order_dev, bs, dev):
    """One epoch as a loop of gather(w=) and step(w=) → every step's {Σ w·lp, W}."""
    import torch

    out = []
    for b0 in range(0, N, bs):
        c = min(bs, N - b0)
        xo = torch.empty(c * d, dtype=torch.float32, device=dev)
        to = torch.empty(c * n, dtype=torch.float32, device=dev) if n else None
        wo = torch.empty(c, dtype=torch.float32, device=dev)
        tr.gather(xo, to, xs, ts, N, order_dev, b0, c, w=(wo, wt))
        ws = _sums(dev)
        tr.step(xo, to, c, w=wo, wsums=ws)
        out.append(ws)
    torch.cuda.synchronize()
    return np.stack([s.cpu().numpy() for s in out])


def test_weighted_epoch_equals_the_gather_and_step_loop(cuda):
    import torch

    _, d, n, x, th = T.case_data("readme")
    _, a = _plain_trainer("readme")
    _, b = _plain_trainer("readme")
    N, bs, steps = 150, 64, 3
    w = (np.random.default_rng(3).random(N) + 0.1).astype(np.float32)
    xs, ts, wt = _dev(x[:, :N], cuda), _dev(th[:, :N], cuda), _wdev(w, cuda)
    od = torch.empty(N, dtype=torch.int32, device=cuda)
    sw = _sums(cuda, 2 * steps)
    rng = np.random.default_rng(5)
    for ep in range(3):                                  # eager, captured, replayed
        order = rng.permutation(N).astype(np.int32)
        od.copy_(torch.from_numpy(order))
        sw.fill_(float("nan"))
        assert a.epoch(xs, ts, N, od, bs, w=wt, step_wsums=sw) == steps
        ref = _hand_epoch(b, xs, ts, wt, N, d, n, od, bs, cuda)
        got = sw.cpu().numpy().reshape(steps, 2)
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), f"epoch {ep}: {got} against {ref}"
        assert E._same_bits(a.get_params(), b.get_params()), f"epoch {ep}: parameters differ"
        want = np.array([np.sum(w[order[i:i + bs]], dtype=np.float64) for i in range(0, N, bs)])
        assert np.all(np.abs(got[:, 1] - want) <= 1e-12 * want), f"epoch {ep}: W {got[:, 1]} against {want}"


def _flow(weights=True):
    """tests/test_gpu_epoch.py's flow (N_train = 150, N_valid = 40, the README chain), with
    real sample weights."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal((5, 190)).astype(np.float32)
    th = (rng.random((1, 190)) * 4.0 - 1.0).astype(np.float32)
    w = (np.random.default_rng(3).random(190) + 0.1).astype(np.float32) if weights else None
    data = dfa.DataArrays(x, th, f_training=150 / 190, f_validation=40 / 190, rng=rng, weights=w)
    chain = dfa.FlowChain(
        dfa.CouplingLayer(data, [1, 2, 3], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.CouplingLayer(data, [3, 4, 5], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.CouplingLayer(data, [5, 1, 2], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
        dfa.NormalizationLayer.from_data(x, -1.0, 1.0))
    flow = dfa.Flow(chain, data)
    assert data.training_data()[0].shape[1] == 150 and data.validation_data()[0].shape[1] == 40
    return data, chain, flow


def test_train_loaders_agree_on_weighted_data(cuda):
    import torch

    out = {}
    for loader in ("host", "device"):
        data, chain, flow = _flow()
        state = setup(Adam(1e-3), flow)
        kw = dict(return_step_losses=True) if loader == "device" else {}
        r = train_(flow, data, state, epochs=3, batchsize=64, shuffle=True, verbose=False,
                   rng=np.random.default_rng(7), loader=loader, **kw)
        out[loader] = (state.trainer.get_params(), list(flow.train_loss), list(flow.valid_loss), r)
    h, dv = out["host"], out["device"]
    assert E._same_bits(dv[0], h[0]), "parameters differ between the loaders"
    assert len(h[1]) == 3 and dv[1] == h[1] and dv[2] == h[2], (dv[1], h[1], dv[2], h[2])
    assert np.all(np.isfinite(h[1])) and np.all(np.isfinite(h[2]))
    res, losses = dv[3]
    assert res is None and losses.shape == (9,) and np.all(np.isfinite(losses))
    # the hand loop: gather(w=) and step(w=) on the same permutations
    data, chain, flow = _flow()
    state = setup(Adam(1e-3), flow)
    tr = state.trainer
    x_tr, th_tr = data.training_data()
    xs, ts, wt = _dev(x_tr, cuda), _dev(th_tr, cuda), _wdev(data.training_weights(), cuda)
    rng = np.random.default_rng(7)
    hand = []
    for ep in range(3):
        od = torch.from_numpy(rng.permutation(150).astype(np.int32)).to(cuda)
        ws = _hand_epoch(tr, xs, ts, wt, 150, 5, 1, od, 64, cuda)
        hand.append(-ws[:, 0] / ws[:, 1])
    assert E._same_bits(tr.get_params(), h[0]), "the hand loop's parameters differ"
    assert np.array_equal(np.concatenate(hand).view(np.int64), losses.view(np.int64)), (hand, losses)
    # unweighted data is another loss
    data, chain, flow = _flow(weights=False)
    state = setup(Adam(1e-3), flow)
    train_(flow, data, state, epochs=1, batchsize=64, verbose=False, rng=np.random.default_rng(7))
    assert flow.train_loss[0] != h[1][0]


# ---- 9. train_ with DataArrays(weights=) ---------------------------------------------------

def test_pushed_losses_are_the_weighted_means(cuda):
    data, chain, flow = _flow()
    state = setup(Adam(1e-3), flow)
    x_tr, th_tr = data.training_data()
    x_va, th_va = data.validation_data()
    rng = np.random.default_rng(7)
    for ep in range(2):
        train_(flow, data, state, epochs=1, batchsize=64, verbose=False, rng=rng)
        lt, Wt = weighted_nll(flow, x_tr, th_tr, data.training_weights())
        lv, Wv = weighted_nll(flow, x_va, th_va, data.validation_weights())
        assert len(flow.train_loss) == ep + 1
        assert flow.train_loss[-1] == lt and flow.valid_loss[-1] == lv, (flow.train_loss, lt, flow.valid_loss, lv)
        assert abs(Wt - np.sum(data.training_weights(), dtype=np.float64)) <= 1e-12 * Wt
    # against numpy on the GPU's per-sample logpdf
    lp = dfa.logpdf(flow, x_tr, th_tr)
    lp = np.asarray(lp.cpu() if hasattr(lp, "cpu") else lp, np.float64)
    w = data.training_weights().astype(np.float64)
    assert abs(flow.train_loss[-1] + np.sum(w * lp) / np.sum(w)) <= 1e-9 * max(1.0, abs(flow.train_loss[-1]))


def test_world_1_comm_run_is_the_local_run(cuda):
    from densityflows_amd.parallel import DFComm

    try:
        comm = DFComm(0)
    except _lib.UnsupportedError as e:           # no RCCL on this machine
        pytest.skip(str(e))
    try:
        out = []
        for c in (None, comm):
            data, chain, flow = _flow()
            state = setup(Adam(1e-3), flow)
            train_(flow, data, state, epochs=2, batchsize=64, verbose=False, rng=np.random.default_rng(7), comm=c)
            out.append((state.trainer.get_params(), list(flow.train_loss), list(flow.valid_loss)))
    finally:
        comm.close()
    assert E._same_bits(out[0][0], out[1][0]), "parameters differ"
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2], out


# ---- 10. df_flow_logpdf_wsum ---------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 257, WSUM_SPAN + 1])
def test_logpdf_wsum_against_numpy(cuda, B):
    import torch

    spec = T.case_data("readme")[0]
    h = spec_to_element(spec).hip()
    x, th = T._inputs(5, 1, B, seed=9)
    w = (np.random.default_rng(3).random(B) + 0.1).astype(np.float32)
    xb, tb, wb = _dev(x, cuda), _dev(th, cuda), _wdev(w, cuda)
    lp = torch.empty(B, dtype=torch.float32, device=cuda)
    lib, stream = h.lib, C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.df_chain_logpdf(h.handle, ptr(xb), ptr(tb), ptr(lp), B, stream))
    for fn in (lib.df_chain_logpdf_wsum,):
        ws = _sums(cuda)
        _lib.check(fn(h.handle, ptr(xb), ptr(tb), ptr(wb), B, ptr(ws), stream))
        torch.cuda.synchronize()
        got = ws.cpu().numpy()
        want = np.sum(w.astype(np.float64) * lp.cpu().numpy().astype(np.float64))
        wantW = np.sum(w, dtype=np.float64)
        assert abs(got[0] - want) <= 1e-12 * abs(want), (B, got[0], want)
        assert abs(got[1] - wantW) <= 1e-12 * wantW, (B, got[1], wantW)
    # df_flow_*: θ raw, normalised with the chain's bounds
    lo, hi = np.array([-1.0], np.float32), np.array([3.0], np.float32)
    _lib.check(lib.df_chain_set_theta_bounds(h.handle, lo.ctypes.data_as(C.POINTER(C.c_float)),
                                             hi.ctypes.data_as(C.POINTER(C.c_float))))
    raw = _dev(th * 4.0 - 1.0, cuda)
    _lib.check(lib.df_flow_logpdf(h.handle, ptr(xb), ptr(raw), ptr(lp), B, stream))
    ws = _sums(cuda)
    _lib.check(lib.df_flow_logpdf_wsum(h.handle, ptr(xb), ptr(raw), ptr(wb), B, ptr(ws), stream))
    torch.cuda.synchronize()
    want = np.sum(w.astype(np.float64) * lp.cpu().numpy().astype(np.float64))
    assert abs(ws.cpu().numpy()[0] - want) <= 1e-12 * abs(want)
    # batch == 0 zeroes both
    ws.fill_(7.0)
    _lib.check(lib.df_flow_logpdf_wsum(h.handle, None, None, None, 0, ptr(ws), stream))
    torch.cuda.synchronize()
    assert np.all(ws.cpu().numpy() == 0.0)


# ---- 11. errors ---------------------------------------------------------------------------

def test_documented_error_codes(cuda):
    import torch

    spec, tr = _plain_trainer("readme")
    _, d, n, x, th = T.case_data("readme")
    lib, B = tr.lib, 16
    xb, tb, wb = _dev(x[:, :B], cuda), _dev(th[:, :B], cuda), _wdev(np.ones(B), cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    p0 = tr.get_params().copy()
    grad_w = lambda w, wt: lib.df_train_gradient_w(tr.handle, ptr(xb), ptr(tb), ptr(w), B, C.c_double(wt), None, stream)
    assert grad_w(None, 0.0) == _lib.DF_ERR_INVALID
    assert grad_w(wb, -1.0) == _lib.DF_ERR_INVALID
    assert grad_w(wb, float("nan")) == _lib.DF_ERR_INVALID
    assert grad_w(wb, 0.0) == _lib.DF_OK
    assert lib.df_train_step_w(tr.handle, ptr(xb), ptr(tb), None, B, None, stream) == _lib.DF_ERR_INVALID
    assert lib.df_train_step_graph_w(tr.handle, ptr(xb), ptr(tb), None, B, C.c_double(0.0), None,
                                     stream) == _lib.DF_ERR_INVALID
    assert lib.df_train_step_graph_w(tr.handle, ptr(xb), ptr(tb), ptr(wb), B, C.c_double(-2.0), None,
                                     stream) == _lib.DF_ERR_INVALID
    assert lib.df_train_epoch_w(tr.handle, ptr(xb), ptr(tb), None, B, None, 8, None, None, stream) == _lib.DF_ERR_INVALID
    # batch == 0: zero gradient, zero wsums
    ws = _sums(cuda)
    ws.fill_(3.0)
    assert lib.df_train_gradient_w(tr.handle, None, None, None, 0, C.c_double(0.0), ptr(ws), stream) == _lib.DF_OK
    torch.cuda.synchronize()
    assert np.all(ws.cpu().numpy() == 0.0) and np.all(tr.grad().cpu().numpy() == 0.0)
    # gather windows
    xo, to, wo = torch.empty(B * d, device=cuda), torch.empty(B * n, device=cuda), torch.empty(B, device=cuda)
    gw = lambda first, count, ns=B: lib.df_batch_gather_w(ptr(xo), ptr(to), ptr(wo), ptr(xb), ptr(tb), ptr(wb), d, n,
                                                          ns, None, first, count, stream)
    assert gw(0, B) == _lib.DF_OK
    assert gw(14, 3) == _lib.DF_ERR_INVALID and gw(-1, 2) == _lib.DF_ERR_INVALID
    assert gw(0, 2, 1 << 31) == _lib.DF_ERR_SHAPE
    assert lib.df_batch_gather_w(ptr(xo), ptr(to), None, ptr(xb), ptr(tb), ptr(wb), d, n, B, None, 0, 2,
                                 stream) == _lib.DF_ERR_INVALID
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tr.get_params().view(np.int32), p0.view(np.int32))
    # with a bad order entry the weight of sample 0 is gathered, like its x and θ
    wset = _wdev(np.arange(1, B + 1), cuda)
    od = torch.tensor([3, B, -1, 5], dtype=torch.int32, device=cuda)
    tr.gather(xo, to, xb, tb, B, od, 0, 4, w=(wo, wset))
    torch.cuda.synchronize()
    assert wo[:4].cpu().tolist() == [4.0, 1.0, 1.0, 6.0]


def test_debug_refuses_an_all_zero_batch(cuda):
    import torch

    spec, tr = _plain_trainer("readme")
    _, d, n, x, th = T.case_data("readme")
    B = 32
    xb, tb = _dev(x[:, :B], cuda), _dev(th[:, :B], cuda)
    tr.set_debug(True)
    p0 = tr.get_params().copy()
    with pytest.raises(_lib.NonFiniteError):
        tr.step(xb, tb, B, w=_wdev(np.zeros(B), cuda))
    with pytest.raises(_lib.NonFiniteError):
        tr.step_graph(xb, tb, B, w=_wdev(np.zeros(B), cuda))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tr.get_params().view(np.int32), p0.view(np.int32))
    tr.step(xb, tb, B, w=_wdev(np.ones(B), cuda))                      # and a good one passes
    torch.cuda.synchronize()
    assert not np.array_equal(tr.get_params(), p0)
