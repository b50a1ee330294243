"""Dump the chain-pass outputs of one library build (DENSITYFLOWS_HIP_LIB) on fixed
seeded inputs, for bitwise A/B comparisons between builds:
    python tools/dump_outputs.py out.npz         # one build
    python tools/dump_outputs.py --compare a.npz b.npz
Workloads: the bench's config-2 and config-4 models (forward, inverse, logpdf) and a
training gradient of each (config 4's is the config-5 sweep); then the trainer's host
code, sweep form by sweep form, on the small chains of tests/test_gpu_train.py
(dump_training: gradients, steps and their repacks, capacity growth, captured steps)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(path):
    import torch

    import bench
    from densityflows_amd.train import Adam, HIPTrainer

    dev = torch.device("cuda", 0)
    out = {}
    for cfg, B in (("cfg2", 1 << 16), ("cfg4", 1 << 12)):
        d, n, _ = bench.CONFIGS[cfg]
        chain = bench.build_chain(cfg)
        hc = chain.hip(device=0, n_hint=n)
        if n:
            hc.set_theta_bounds(np.zeros(n, np.float32), np.ones(n, np.float32))
        g = torch.Generator(device=dev).manual_seed(7)
        z = torch.randn(B * d, device=dev, generator=g)
        th = torch.rand(B * n, device=dev, generator=g) if n else None
        x, ldj = torch.empty_like(z), torch.empty(B, device=dev)
        hc.run("forward", z, th, x, ldj, B)
        zb, ldjb = torch.empty_like(z), torch.empty(B, device=dev)
        hc.run("backward", x, th, zb, ldjb, B)
        lp = torch.empty(B, device=dev)
        hc.run_logpdf(x, th, lp, B)
        for k, v in (("x", x), ("ldj", ldj), ("zb", zb), ("ldjb", ldjb), ("lp", lp)):
            out[f"{cfg}_{k}"] = v.cpu().numpy()
        tr = HIPTrainer(hc, Adam(1e-3))  # cfg4: the config-5 sweep (wide inverse pass)
        tr.gradient(x, th, B, B)
        torch.cuda.synchronize()
        out[f"{cfg}_grad"] = tr.grad().cpu().numpy()
        del tr
    dump_training(out, dev)
    np.savez(path, **out)
    print("dumped", path, f"({len(out)} arrays)")


def _train_entries():
    """(key, spec builder, d, n, sweep, batch): every sweep form of the trainer's host code
    on the chains of tests/test_gpu_train.py, at batches below, across and off the tiles."""
    import test_gpu_train as T
    from densityflows_amd import train as M
    from helpers import _single_dense_spec
    from oracle import flow_oracle as O

    def softplus_spec(rng):  # hidden σ with a kept pre-activation (LNet::pre, the σ'(x) buffers)
        return {"kind": "chain", "layers": [
            O.rnvp_layer(rng, O.coupling_axes(5, [1, 2, 3], n=1), hidden=16, act="softplus", bias_scale=0.1,
                         out_scale=0.5),
            O.coupling_block(rng, O.coupling_axes_cut(5, 2, n=1), n_sub=1, hidden=32, act="softplus",
                             bias_scale=0.1, out_scale=0.5)]}

    sep = M.SWEEP_LAYERWISE | M.SWEEP_SEPARATE
    forms = {"readme": ((M.SWEEP_AUTO, M.SWEEP_LAYERWISE), (17, 777)),
             "mixed": ((M.SWEEP_AUTO, M.SWEEP_LAYERWISE), (17, 777)),
             "wide": ((M.SWEEP_AUTO, M.SWEEP_RECOMPUTE, sep), (5, 700)),
             "cfg5": ((M.SWEEP_AUTO, M.SWEEP_KEPT, M.SWEEP_RECOMPUTE, sep), (5, 300, 777)),
             "cfg5_in40": ((M.SWEEP_AUTO,), (300,)),   # the x̄-apart fallback
             "nobias": ((M.SWEEP_LAYERWISE,), (17,))}
    entries = [(f"{name}_s{sw}_B{B}",) + T.SPECS[name] + (sw, B)
               for name, (sweeps, batches) in forms.items() for sw in sweeps for B in batches]
    entries.append((f"softplus_s{M.SWEEP_LAYERWISE}_B777", softplus_spec, 5, 1, M.SWEEP_LAYERWISE, 777))
    entries.append((f"single_dense_s{M.SWEEP_AUTO}_B17", _single_dense_spec, 5, 1, M.SWEEP_AUTO, 17))
    return entries


def dump_training(out, dev, grow_to=3001):
    """Per entry: gradient and Σ logpdf; parameters after 3 steps (every repack map) and the
    chain's forward output on them; the gradient after growing the trainer to grow_to samples;
    parameters after 3 step_graph calls; on the fused sweep, logpdf_grad's outputs."""
    import torch

    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from densityflows_amd import train as M
    from helpers import spec_to_element

    def inputs(d, n, B, seed):
        rng = np.random.default_rng(seed)
        x = torch.from_numpy(rng.standard_normal(B * d).astype(np.float32)).to(dev)
        th = torch.from_numpy(rng.random(B * n).astype(np.float32)).to(dev) if n else None
        return x, th

    for key, make, d, n, sweep, B in _train_entries():
        hc = spec_to_element(make(np.random.default_rng(0))).hip()
        tr = M.HIPTrainer(hc, M.Adam(1e-3), sweep=sweep)
        x, th = inputs(d, n, B, 1)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)

        def grad_of(x, th, B, tag):
            tr.gradient(x, th, B, B, lp)
            torch.cuda.synchronize()
            out[f"{key}_{tag}"] = tr.grad().cpu().numpy().copy()
            out[f"{key}_{tag}_lp"] = lp.cpu().numpy()

        grad_of(x, th, B, "grad")
        out[f"{key}_form"] = np.array([tr.sweep()], np.int32)
        for _ in range(3):
            tr.step(x, th, B)
        out[f"{key}_params"] = tr.get_params()
        y, ldj = torch.empty_like(x), torch.empty(B, device=dev)
        hc.run("forward", x, th, y, ldj, B)
        torch.cuda.synchronize()
        out[f"{key}_fwd"], out[f"{key}_fwd_ldj"] = y.cpu().numpy(), ldj.cpu().numpy()
        grad_of(*inputs(d, n, grow_to, 2), grow_to, "grown")
        for _ in range(3):  # eager, then captured, then replayed
            tr.step_graph(x, th, B)
        out[f"{key}_graph_params"] = tr.get_params()
        if tr.sweep() == M.SWEEP_FUSED:
            lps, gx = torch.empty(B, device=dev), torch.empty_like(x)
            gth = torch.empty(B * n, device=dev) if n else None
            tr.logpdf_grad(x, th, B, lps, gx, gth)
            torch.cuda.synchronize()
            out[f"{key}_score_lp"], out[f"{key}_score_gx"] = lps.cpu().numpy(), gx.cpu().numpy()
            if n:
                out[f"{key}_score_gth"] = gth.cpu().numpy()
        tr.close()
        print("trained", key, flush=True)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    same = True
    for k in sorted(A.files):
        eq = np.array_equal(A[k].view(np.uint32), Bz[k].view(np.uint32))
        diff = np.max(np.abs(A[k].astype(np.float64) - Bz[k])) if not eq else 0.0
        print(f"{k:32s} {'bitwise-identical' if eq else 'DIFFERS max|Δ| %.3g' % diff}")
        same &= eq
    print("ALL BITWISE IDENTICAL" if same else "DIFFERENT")
    return same


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    dump(sys.argv[1])
