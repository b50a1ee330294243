"""A non-finite sample stays local, in every chain-pass kernel family and in the per-sample
score kernel ("activation ladder and isolation matrix").

tests/test_gpu_split_rem.py::test_nonfinite_sample_stays_local holds this for one kernel,
one sample and no θ.  Here: the eleven chains of tests/edge_cases.py with their
environments and inputs, at B = G + 17 (G: the samples of one wave's tile group at the
unforced plan; 49 for the wide kernels): one full group and a ragged tile with idle lanes.

One sample is poisoned at a time — 0, 5, 15, 16 (the first of a second tile), G − 1, G (the
first of the ragged tile), B − 1 — in one element: the first conditioner feature of the
first layer, a transformed dim of the first layer, or a θ column.  Values: +qNaN
(0x7FC00000) at every sample and element; +inf, −inf and 3e38 at samples 5, G − 1, B − 1;
the negative quiet NaN 0xFFC00000 at sample 5.  Entry points: forward, forward!, inverse and
logpdf, and df_train_logpdf_grad for the chains the fused training class takes.

 1. Every other sample's outputs are bitwise those of the clean run, and finite.
 2. +NaN: the non-finite output elements of the poisoned sample are those of the float32
    oracle on the same input (numpy's maximum propagates NaN as Julia's max does): what is
    downstream of the NaN is NaN, nothing upstream is.
 3. ±inf, 3e38: the poisoned sample's logpdf is non-finite wherever the float32 oracle's
    is (element patterns are not compared: the bf16x3 split turns an inf into inf − inf).
 −NaN: assertions 1 and 2.

Outcome.  A NaN from an x86 host (0f0/0f0, log(-1)) has the sign bit set, and on
the device x − t and −s flip the sign of a NaN they are handed, so sign-set NaNs occur
inside a chain whatever the input's sign.  relu as one integer maximum of the bit pattern
orders such a NaN below zero and returns +0.  With that relu in every kernel this file
failed assertion 2 for both NaNs in the generic kernel on relu Denses and in the
specialised relu, FAST, SPLIT and wide kernels (FAST exact, +NaN in x[0]: inverse z
non-finite [1 0 1 1 1], oracle [1 1 1 1 1]; wide SPLIT: forward x [1 0 0 0 0 0] against all
six) and assertion 3 for θ (θ = +inf: a finite logpdf of −25.4 on the d = 12 chain, −11.8
on the wide exact kernel).  With the IEEE maximum (one v_maximum3_f32) everywhere, every
chain-pass assertion here passed, but config 2 ran 1.1959–1.1978 M cycles per launch
against the parent's 1.1912–1.1942 in three alternations: outside the parent's spread.
So the generic kernel's relu is the IEEE maximum and the generic chains are held to
assertions 2 and 3 as written, as are the chains without relu; the kernels on
uni::relu_fast keep the integer maximum, and their chains are held to what is documented:
assertion 1; nothing is non-finite that the oracle keeps finite; a poisoned state dim is
NaN in x, forward!, z and the logpdf; assertion 3 for a poisoned state dim.  A non-finite
θ may leave such a chain with finite outputs.  The score kernel's gθ of a NaN sample is
finite on the relu chains (its σ′ mask selects) where the oracle's NaN·0 is NaN.

These inputs are values, not faults: the chain-pass, training and score kernels index by
lane, tile and plan tables only; no address is computed from sample data.
"""
import numpy as np
import pytest

import edge_cases as E
import score_ref as R
from densityflows_amd import _lib
from densityflows_amd.train import Adam, HIPTrainer
from oracle import flow_oracle as O
from test_gpu_batch_edges import _Handle, _launches

pytestmark = pytest.mark.gpu

POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
BIG = int(np.float32(3e38).view(np.uint32))
SCORE_CHAINS = ("fast16", "split64", "split32", "uniform_tanh32")
PASS_KEYS = ("x", "ldj", "x_inplace", "z", "ldj_b", "lp")
SCORE_KEYS = ("s_lp", "s_gx", "s_gth")


def _bits(v):
    return np.array([v], np.uint32).view(np.float32)[0]


class _Runner:
    """The entry points of one case on device copies of its first B samples."""

    def __init__(self, H, B, score):
        self.H, self.B, D = H, B, H.D
        self.d, self.n = D["d"], D["n"]
        self.z, self.x = H.zin[:B * self.d].clone(), H.xin[:B * self.d].clone()
        self.th = {k: (v[:B * self.n].clone() if v is not None else None) for k, v in H.th.items()}
        self.tr = None
        if score:
            self.tr = HIPTrainer(H.h, Adam())
            self.tr.set_theta_input(_lib.DF_THETA_GIVEN)

    def run(self, poison=None):
        """poison: (sample, "x" | "theta", row, uint32 bits) or None → {key: array, sample first}."""
        import torch

        B, d, n, h, dev = self.B, self.d, self.n, self.H.h, self.H.dev
        z, x, th, thr = self.z, self.x, self.th[False], self.th[True]
        if poison is not None:
            smp, where, row, bits = poison
            val = int(np.array([bits], np.uint32).view(np.int32)[0])
            if where == "x":
                z, x = z.clone(), x.clone()
                z.view(torch.int32)[smp * d + row] = val
                x.view(torch.int32)[smp * d + row] = val
            else:
                th, thr = th.clone(), thr.clone()
                th.view(torch.int32)[smp * n + row] = val
                thr.view(torch.int32)[smp * n + row] = val
        new = lambda rows: torch.zeros(B * rows, dtype=torch.float32, device=dev)
        xb, lb, zb, lbb, lp = new(d), new(1), new(d), new(1), new(1)
        h.run("forward", z, th, xb, lb, B, False)
        zz = z.clone()
        h.run_inplace(zz, th, B, False)
        h.run("backward", x, th, zb, lbb, B, False)
        h.run_logpdf(x, thr, lp, B)
        out = {"x": (xb, d), "ldj": (lb, 1), "x_inplace": (zz, d), "z": (zb, d), "ldj_b": (lbb, 1), "lp": (lp, 1)}
        if self.tr is not None:
            slp, sgx, sgt = new(1), new(d), (new(n) if n else None)
            self.tr.logpdf_grad(x, th, B, slp, sgx, sgt)
            out.update(s_lp=(slp, 1), s_gx=(sgx, d))
            if n:
                out["s_gth"] = (sgt, n)
        torch.cuda.synchronize()
        return {k: b.cpu().numpy().reshape(B, rows) for k, (b, rows) in out.items()}


def _oracle_masks(D, variants, score):
    """The float32 oracle on one column per variant → {key: non-finite mask (variants, rows)}.
    The logpdf sees the raw θ normalised, as the kernel does."""
    d, n = D["d"], D["n"]
    V = len(variants)
    Z, X = np.empty((d, V), np.float32), np.empty((d, V), np.float32)
    TH, THR = np.empty((n, V), np.float32), np.empty((n, V), np.float32)
    for j, (smp, where, row, bits) in enumerate(variants):
        Z[:, j], X[:, j], TH[:, j], THR[:, j] = D["z"][:, smp], D["x_in"][:, smp], D["th"][:, smp], D["th_raw"][:, smp]
        if where == "x":
            Z[row, j] = X[row, j] = _bits(bits)
        else:
            TH[row, j] = THR[row, j] = _bits(bits)
    spec = D["spec"]
    with np.errstate(all="ignore"):
        x, ldj = O.forward(spec, Z, TH, np.float32)
        zb, ldj_b = O.backward(spec, X, TH, np.float32)
        thn = O.normalize_input(THR, D["tmin"], D["tmax"]) if n else THR
        lp = O.flow_logpdf(spec, X, thn, np.float32)
        out = {"x": x.T, "ldj": ldj[:, None], "x_inplace": x.T, "z": zb.T, "ldj_b": ldj_b[:, None], "lp": lp[:, None]}
        if score:
            slp, gx, gth, _ = R.logpdf_grad(spec, X, TH, dtype=np.float32)
            out.update(s_lp=slp[:, None], s_gx=gx.T)
            if n:
                out["s_gth"] = gth.T
    return {k: ~np.isfinite(v) for k, v in out.items()}


def _check_others(clean, dirty, smp, what):
    """Assertion 1."""
    others = np.arange(next(iter(clean.values())).shape[0]) != smp
    for k, v in clean.items():
        a, b = v[others], dirty[k][others]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{what}: {k} of other samples changed (rows {np.argwhere(np.any(a.view(np.uint32) != b.view(np.uint32), axis=1))[:4].ravel()})"


def _has_relu(spec):
    return any(D["act"] == "relu" for L in O._flat_layers(spec) if L["kind"] != "norm"
               for net in ("s_net", "t_net") for D in L.get(net, []))


@pytest.mark.parametrize("name", list(E.CASES))
def test_nonfinite_sample_stays_local(cuda, name, monkeypatch, capfd):
    _, d, n, _, kernel_ids, group, _ = E.CASES[name]
    wide = name in E.WIDE
    G = 16 * group
    B = 49 if wide else G + 17
    H = _Handle(name, 0, monkeypatch, cuda)
    kid = H.h.info.kernel
    assert kid in kernel_ids, f"{name} planned kernel {kid}, expected one of {kernel_ids}"
    D, score = H.D, name in SCORE_CHAINS
    run = _Runner(H, B, score)

    capfd.readouterr()
    clean = run.run()
    seen = _launches(capfd)
    assert len(seen) == 4 + score, seen           # (the score call runs one chain pass of its own)
    for nm, t, mx in seen:
        assert nm == E.KERNEL_NAME[kid] and (wide or t == group), f"{name}: launched {nm} at {t} tiles per wave"
    for k, v in clean.items():
        assert np.all(np.isfinite(v)), f"{name}: clean {k} is not finite"
    assert set(clean) == set(PASS_KEYS) | (set(SCORE_KEYS[:2 + (n > 0)]) if score else set())

    L0 = D["spec"]["layers"][0]
    elements = [("x", L0["axis_id"][0] - 1), ("x", L0["axis_af"][0] - 1)] + ([("theta", 0)] if n else [])
    everywhere = sorted({0, 5, 15, 16, G - 1, G, B - 1})
    some = sorted({5, G - 1, B - 1})
    variants = [(s, w, r, POS_NAN) for s in everywhere for w, r in elements]
    variants += [(s, w, r, v) for v in (POS_INF, NEG_INF, BIG) for s in some for w, r in elements]
    variants += [(5, w, r, NEG_NAN) for w, r in elements]
    assert all(0 <= s < B for s, _, _, _ in variants)
    want = _oracle_masks(D, variants, score)
    strict = kid == 0 or not _has_relu(D["spec"])
    kept, asked = [0, 0], [0, 0]

    for j, (smp, where, row, bits) in enumerate(variants):
        what = f"{name} sample {smp} {where}[{row}] = {bits:#010x}"
        dirty = run.run((smp, where, row, bits))
        _check_others(clean, dirty, smp, what)
        wj = {k: m[j] for k, m in want.items()}
        if bits in (POS_NAN, NEG_NAN):
            same = True
            for k, v in dirty.items():
                got = ~np.isfinite(v[smp])
                assert np.all(np.isnan(v[smp][got])), f"{what}: {k} downstream of the NaN is not NaN"
                assert not np.any(got & ~wj[k]), f"{what}: non-finite {k} {got.astype(int)}, oracle {wj[k].astype(int)}"
                if strict:
                    assert np.array_equal(got, wj[k]), f"{what}: non-finite {k} {got.astype(int)}, oracle {wj[k].astype(int)}"
                same = same and np.array_equal(got, wj[k])
            kept[bits == NEG_NAN] += same
            asked[bits == NEG_NAN] += 1
            if where == "x":        # what DESIGN §7 documents of the kernels on uni::relu_fast (and holds of all)
                for k in ("x", "x_inplace", "z"):
                    assert np.isnan(dirty[k][smp, row]), f"{what}: {k}[{row}] is not NaN"
                for k in ("lp", "s_lp"):
                    assert k not in dirty or np.isnan(dirty[k][smp, 0]), f"{what}: {k} is not NaN"
        elif strict or where == "x":
            for k in ("lp", "s_lp"):
                if k in dirty and wj[k][0]:
                    assert not np.isfinite(dirty[k][smp, 0]), f"{what}: {k} is finite, the float32 oracle's is not"
    capfd.readouterr()
    print(f"NONFINITE {name}: kernel {kid} B {B} G {G}, {len(variants)} poisoned runs, "
          f"{'held to' if strict else 'documented apart from'} the oracle's NaN pattern: kept in {kept[0]} of {asked[0]} "
          f"+NaN and {kept[1]} of {asked[1]} -NaN runs")
