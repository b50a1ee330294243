"""The activation ladder on the device ("activation ladder and isolation matrix").

The other parity tests keep every conditioner pre-activation within a few units of zero.
The chains of tests/act_ladder_cases.py carry the branch points of the non-relu activation
code in their biases (tanh_fast's x² = 66, sigmoid_fast's 40 and −80, the overflow range of
exp and cosh, |x| ≈ 1e-3); tests/test_act_ladder_host.py shows on the CPU that every case
visits every branch, that the oracle's own float32 evaluation keeps half the tolerances
below, and that four plausible wrong activations fail them.

Chain passes: every case runs forward, forward! and inverse at chain and flow level, the
per-sample logpdf and its fp64 sum on raw buffers (test_gpu_batch_edges._Handle's run), at a
batch with a ragged second trip (257; 145 for the MFMA output path), and is held to
  * values: `close(·, fp64 oracle, 1e-5)`;
  * finiteness: all B rows finite, the NaN-patterned guard rows behind every output untouched;
  * kernel id: the df_chain_info.kernel the case names, or the case tests nothing.
Gradients (smooth activations; `DF_GRID_CUS=2`, B = 300: past one trip of the fused kernel
at one workgroup per CU, past two of the score kernel): df_train_gradient against
O.nll_and_grad under G_RTOL / G_ATOL per tensor with the loss to 1e-5, on the sweep form the
case names (fused; kept and recomputed H for the hidden-128 three-hidden-Dense nets), and
df_train_logpdf_grad's lp, gx, gθ against score_ref.logpdf_grad under the same tolerances.
"""
import numpy as np
import pytest

import act_ladder_cases as A
import densityflows_amd.train as train_mod
from densityflows_amd import _lib
from densityflows_amd.train import Adam, HIPTrainer
from helpers import close, spec_to_element
from test_gpu_batch_edges import ENV_KEYS, _Handle, _flat
from test_gpu_train_edges import ENV_KEYS as TRAIN_ENV_KEYS, TRAIN_LINE, _same_bits

pytestmark = pytest.mark.gpu

PAD = 2 * 128 + 7


class _LadderHandle(_Handle):
    """test_gpu_batch_edges._Handle on a case of the ladder."""

    def __init__(self, name, monkeypatch, cuda):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in A.CHAIN_CASES[name][4].items():
            monkeypatch.setenv(k, v)
        self.D = D = A.case_data(name)
        self.dev = cuda
        self.h = spec_to_element(D["spec"]).hip()
        self.h.set_theta_bounds(D["tmin"], D["tmax"])
        self.zin, self.xin = _flat(D["z"], cuda), _flat(D["x_in"], cuda)
        self.th = {False: _flat(D["th"], cuda), True: _flat(D["th_raw"], cuda)}


@pytest.mark.parametrize("name", list(A.CHAIN_CASES))
def test_chain_passes(cuda, name, monkeypatch):
    ids = A.CHAIN_CASES[name][5]
    H = _LadderHandle(name, monkeypatch, cuda)
    kid = H.h.info.kernel
    assert kid in ids, f"{name} planned kernel {kid}, expected one of {ids} ({A.CHAIN_CASES[name][6]})"
    B = H.D["B"]
    out = H.run(B, PAD)                 # finiteness and guards: _Handle._take
    worst = H.check_values(out, B)      # values, at chain and flow level
    print(f"LADDER {name}: kernel {kid} B {B} worst ratio " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _trainer(name, monkeypatch, capfd):
    spec = A.grad_data(name)["spec"]
    _, sweep, form, _ = A.GRAD_CASES[name]
    for k in TRAIN_ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
    monkeypatch.setenv("DF_GRID_CUS", str(A.TRAIN_GRID_CUS))
    capfd.readouterr()
    tr = HIPTrainer(spec_to_element(spec).hip(), Adam(), sweep=getattr(train_mod, "SWEEP_" + sweep))
    lines = TRAIN_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, (name, lines)
    word, cus, n_cu, grid, occ, lgrid = lines[0]
    assert int(cus) == A.TRAIN_GRID_CUS, f"{name}: grids sized from {cus} CUs"
    assert tr.sweep() == getattr(train_mod, "SWEEP_" + form), f"{name}: sweep form {tr.sweep()}, expected {form}"
    assert word == ("fused" if form == "FUSED" else "layer-wise"), (name, word)
    return tr, int(grid), int(occ)


@pytest.mark.parametrize("name", list(A.GRAD_CASES))
def test_gradient(cuda, name, monkeypatch, capfd):
    import torch

    D = A.grad_data(name)
    spec, B = D["spec"], D["B"]
    tr, grid, occ = _trainer(name, monkeypatch, capfd)
    x, th = _flat(D["x"], cuda), _flat(D["th"], cuda)
    lp = torch.zeros(1, dtype=torch.float64, device=cuda)
    tr.gradient(x, th, B, B, lp)
    torch.cuda.synchronize()
    g, lpsum = tr.grad().detach().cpu().numpy().copy(), float(lp.item())
    tr.gradient(x, th, B, B, lp)
    torch.cuda.synchronize()
    assert _same_bits(g, tr.grad().detach().cpu().numpy()) and lpsum == float(lp.item()), f"{name}: two evaluations differ"
    assert np.all(np.isfinite(g)) and np.isfinite(lpsum), f"{name}: non-finite gradient or Σ logpdf"
    assert g.shape == D["grad"].shape
    r_loss = abs(-lpsum / B - D["loss"]) / (1e-5 * max(1.0, abs(D["loss"])))
    ratios = [close(g[sl], D["grad"][sl], A.G_RTOL, A.G_ATOL)[1] for sl in A._tensor_slices(spec)]
    capfd.readouterr()
    print(f"LADDER {name}: {A.GRAD_CASES[name][2]} grid {grid} occ {occ} B {B} worst ratio grad {max(ratios):.3f} "
          f"loss {r_loss:.3f}")
    assert r_loss <= 1.0, f"{name}: loss {-lpsum / B} against {D['loss']}"
    assert max(ratios) <= 1.0, f"{name}: gradient violation ratio {max(ratios)}"


@pytest.mark.parametrize("name", list(A.SCORE_CASES))
def test_score(cuda, name, monkeypatch, capfd):
    import torch

    D = A.grad_data(name)
    d, n, B = D["d"], D["n"], D["B"]
    tr, _, _ = _trainer(name, monkeypatch, capfd)
    tr.set_theta_input(_lib.DF_THETA_GIVEN)
    nan = lambda rows: torch.full((B * rows,), float("nan"), dtype=torch.float32, device=cuda)
    lpb, gxb, gtb = nan(1), nan(d), nan(n)
    tr.logpdf_grad(_flat(D["x"], cuda), _flat(D["th"], cuda), B, lpb, gxb, gtb)
    torch.cuda.synchronize()
    lp = lpb.cpu().numpy()
    gx, gth = gxb.cpu().numpy().reshape(B, d).T, gtb.cpu().numpy().reshape(B, n).T
    assert all(np.all(np.isfinite(a)) for a in (lp, gx, gth)), f"{name}: non-finite score output"
    ratios = {"lp": close(lp, D["lp"])[1], "gx": close(gx, D["gx"], A.G_RTOL, A.G_ATOL)[1],
              "gth": close(gth, D["gth"], A.G_RTOL, A.G_ATOL)[1]}
    capfd.readouterr()
    print(f"LADDER score {name}: B {B} worst ratio " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, f"{name}: violation ratios {ratios}"
