"""Pinned bits of the SPLIT kernels (tests/test_gpu_split_rem.py::test_pinned_bits).

The bf16x3 activation split and the output GEMV of the specialised SPLIT kernel
(densityflows.jl_amd/csrc/df_uniform_impl.h) may be re-scheduled or moved to other
instructions, but every rounding stays where it is, so their outputs are pinned bit for
bit.  This generator needs an MI355X and the built library; it wrote the committed
``split_pin_*.npy`` on commit

    38404ad  (bench: lean plain run, --full for secondary legs, --dump-outputs)

that is, on the build BEFORE the remainders moved from v_mfma_f32_16x16x16_bf16 to
v_mfma_f32_4x4x4_16b_bf16.  Regenerate only when a change is MEANT to alter the
arithmetic, and state the commit here (``python tests/golden/make_split_pin.py --commit <sha>`` also records it in
split_pin_meta.json).

Cases (B = 600: one 512-sample workgroup plus a partial one; inputs from numpy seeds):
  config-2 chain (bench.build_chain("cfg2")): forward x / ldj of z, inverse x / ldj and
  logpdf of the pinned forward x;
  one CouplingBlock, d = 5, hidden 64: the gradient of one HIPTrainer.gradient call.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 600
D = 5
NAMES = ("fwd_x", "fwd_ldj", "inv_x", "inv_ldj", "logpdf", "grad")


def path(name):
    return os.path.join(HERE, f"split_pin_{name}.npy")


def inputs():
    """z (B·d, sample-major: Julia's (d, B) column-major) and the training batch."""
    z = np.random.default_rng(20261).standard_normal((B, D)).astype(np.float32).reshape(-1)
    xt = np.random.default_rng(20262).standard_normal((B, D)).astype(np.float32).reshape(-1)
    return z, xt


def block_chain():
    import densityflows_amd as dfa

    rng = np.random.default_rng(11)
    return dfa.FlowChain.repeat(dfa.CouplingBlock, 1, D, hidden_dim_s=64, hidden_dim_t=64, rng=rng)


def compute(fwd_x=None):
    """Every pinned array from the loaded library.  fwd_x: the input of the inverse and
    logpdf passes (the test passes the pinned forward x, the generator its own)."""
    import torch

    import bench
    from densityflows_amd.train import Adam, HIPTrainer

    dev = torch.device("cuda", 0)
    z, xt = inputs()
    hc = bench.build_chain("cfg2").hip(device=0, n_hint=0)
    assert hc.info.kernel == 4, hc.info.kernel  # the specialised SPLIT kernel
    tz = torch.from_numpy(z).to(dev)
    x, ldj = torch.empty_like(tz), torch.empty(B, device=dev)
    hc.run("forward", tz, None, x, ldj, B)
    out = {"fwd_x": x.cpu().numpy(), "fwd_ldj": ldj.cpu().numpy()}
    tx = torch.from_numpy(out["fwd_x"] if fwd_x is None else fwd_x).to(dev)
    zb, ldjb, lp = torch.empty_like(tx), torch.empty(B, device=dev), torch.empty(B, device=dev)
    hc.run("backward", tx, None, zb, ldjb, B)
    hc.run_logpdf(tx, None, lp, B)
    out.update(inv_x=zb.cpu().numpy(), inv_ldj=ldjb.cpu().numpy(), logpdf=lp.cpu().numpy())
    tr = HIPTrainer(block_chain().hip(device=0, n_hint=0), Adam())
    tr.gradient(torch.from_numpy(xt).to(dev), None, B, B)
    torch.cuda.synchronize()
    out["grad"] = tr.grad().cpu().numpy().copy()
    return out


def main():
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unstated"
    out = compute()
    total = 0
    for k in NAMES:
        assert np.all(np.isfinite(out[k])), k
        np.save(path(k), out[k])
        total += os.path.getsize(path(k))
    with open(os.path.join(HERE, "split_pin_meta.json"), "w") as f:
        json.dump({"commit": commit, "B": B, "shapes": {k: list(out[k].shape) for k in NAMES}}, f, indent=1)
        f.write("\n")
    print("wrote", {k: out[k].shape for k in NAMES}, total, "bytes, commit", commit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
