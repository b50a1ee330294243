"""Batch edges and tiles per wave of every chain-pass kernel ("edge matrix").

One small chain per kernel family (tests/edge_cases.py), each at the batches around its
workgroup size S — 0, 1, 17, S − 1, S, S + 1 (a last workgroup of one sample and seven
idle waves), S + 16 (a wave with one full tile and an empty rest of its tile group) and
2S + 33 — and at the tile counts `DF_TILES` forces: unset (one tile group), 4 and the
plan's maximum, the two sides of the copy-in's kBlockThreads-row boundary.  Every entry
point (forward, forward!, inverse at chain and flow level; per-sample logpdf and its
fp64 sum) runs on raw buffers through HIPChain.run*, and every call is held to:

 1. values: `close(·, fp64 oracle, 1e-5)`, the criterion of test_gpu_parity.py (the
    fp32 oracle keeps it on these weights: test_oracle.py::test_edge_cases_fp32_oracle);
 2. prefix: the outputs at batch B are bitwise the first B samples of the same handle's
    outputs at 2S + 33 — a sample's arithmetic does not depend on its neighbours;
 3. geometry: the outputs of a forced tile count are bitwise those of the unforced plan;
 4. guards: every output buffer is 2S + 7 rows longer than the batch and pre-filled with
    one NaN bit pattern; after the call the pad still holds it and all B rows are finite
    (the fp64 sum is the middle of three doubles whose neighbours must not change).

Only allocated memory is touched: inputs are prefixes of the full-size arrays.
"""
import re

import numpy as np
import pytest

import edge_cases as E
from helpers import close, spec_to_element

pytestmark = pytest.mark.gpu

RTOL = 1e-5
NAN32 = 0x7FC0DEAD                 # a quiet NaN with a recognisable payload
NAN64 = 0x7FF8DEADBEEF0001
ENV_KEYS = ("DF_TILES", "DF_SMALL_MAX", "DF_SMALL_WAVES", "DF_F32_EXACT", "DF_NO_WIDE", "DF_FORCE_GENERIC",
            "DF_NO_FAST", "DF_NO_FOLD", "DF_DEBUG_LAUNCH")
LAUNCH = re.compile(r"\[df\] mode (\d+) batch (\d+) kernel (\S+) tiles (\d+) \(max (\d+)\)")
QUANTITIES = ("x", "ldj", "x_inplace", "z", "ldj_b")


def _params():
    out = []
    for name, (_, _, _, _, _, group, max_tiles) in E.CASES.items():
        out.append((name, "auto"))
        if name in E.WIDE:
            continue
        out.append((name, "max"))
        if max_tiles > 4:
            out.append((name, "t4"))
    return out


def _flat(a, dev):
    """numpy (rows, B) → flat device buffer in Julia memory order (sample-major)."""
    import torch

    return torch.from_numpy(np.array(np.asarray(a, np.float32).T, order="C").ravel()).to(dev)


class _Handle:
    """One df_chain of a case with its inputs on the device."""

    def __init__(self, name, tiles, monkeypatch, cuda):
        entry = E.CASES.get(name)
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (entry[3] if entry else {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
        if tiles:
            monkeypatch.setenv("DF_TILES", str(tiles))
        self.D = D = E.case_data(name)
        self.dev = cuda
        self.h = spec_to_element(D["spec"]).hip()     # a fresh handle: the plan reads the env at creation
        if D["n"]:
            self.h.set_theta_bounds(D["tmin"], D["tmax"])
        self.zin, self.xin = _flat(D["z"], cuda), _flat(D["x_in"], cuda)
        self.th = {False: _flat(D["th"], cuda) if D["n"] else None,
                   True: _flat(D["th_raw"], cuda) if D["n"] else None}

    def _guarded(self, rows, B, pad):
        import torch

        return torch.full(((B + pad) * rows,), NAN32, dtype=torch.int32, device=self.dev).view(torch.float32)

    @staticmethod
    def _take(buf, rows, B, what):
        """The B valid samples of a guarded buffer as (rows, B); the pad must be untouched."""
        import torch

        raw = buf.view(torch.int32).cpu().numpy()
        assert np.all(raw[B * rows:] == NAN32), f"{what}: written past the batch (B = {B})"
        val = raw[:B * rows].view(np.float32)
        assert np.all(np.isfinite(val)), f"{what}: non-finite output (B = {B})"
        return val.reshape(B, rows).T.copy() if rows > 1 else val.copy()

    def run(self, B, pad):
        """Every entry point at batch B → {(quantity, flow): array}, "lp", "sum"."""
        import torch

        d, h, out = self.D["d"], self.h, {}
        for flow in (False, True):
            tag = "flow" if flow else "chain"
            xb, lb = self._guarded(d, B, pad), self._guarded(1, B, pad)
            h.run("forward", self.zin, self.th[flow], xb, lb, B, flow)
            out["x", flow] = self._take(xb, d, B, f"{tag} forward x")
            out["ldj", flow] = self._take(lb, 1, B, f"{tag} forward ldj")
            zz = self._guarded(d, B, pad)
            zz[:B * d] = self.zin[:B * d]
            h.run_inplace(zz, self.th[flow], B, flow)
            out["x_inplace", flow] = self._take(zz, d, B, f"{tag} forward!")
            zb, lb = self._guarded(d, B, pad), self._guarded(1, B, pad)
            h.run("backward", self.xin, self.th[flow], zb, lb, B, flow)
            out["z", flow] = self._take(zb, d, B, f"{tag} inverse z")
            out["ldj_b", flow] = self._take(lb, 1, B, f"{tag} inverse ldj")
        lp = self._guarded(1, B, pad)
        h.run_logpdf(self.xin, self.th[True], lp, B)
        out["lp"] = self._take(lp, 1, B, "logpdf")
        sb = torch.full((3,), NAN64, dtype=torch.int64, device=self.dev).view(torch.float64)
        h.run_logpdf_sum(self.xin, self.th[True], sb[1:2], B)
        raw = sb.view(torch.int64).cpu().numpy()
        assert raw[0] == NAN64 and raw[2] == NAN64, f"logpdf sum: neighbours written (B = {B})"
        out["sum"] = float(raw.view(np.float64)[1])
        torch.cuda.synchronize()
        return out

    def check_values(self, out, B):
        """Assertion 1 at batch B; returns the violation ratios of (x, ldj, z, lp)."""
        D = self.D
        ref = {"x": D["x"], "ldj": D["ldj"], "x_inplace": D["x"], "z": D["zb"], "ldj_b": D["ldj_b"]}
        worst = dict(x=0.0, ldj=0.0, z=0.0, lp=0.0)
        for flow in (False, True):
            for q in QUANTITIES:
                got, want = out[q, flow], ref[q][..., :B]
                assert got.shape == want.shape, (q, flow, got.shape, want.shape)
                ok, r = close(got, want, RTOL)
                assert ok, f"{q} ({'flow' if flow else 'chain'} level) at B = {B}: violation ratio {r}"
                key = {"x_inplace": "x", "ldj_b": "ldj"}.get(q, q)
                worst[key] = max(worst[key], r)
        ok, r = close(out["lp"], D["lp"][:B], RTOL)
        assert ok, f"logpdf at B = {B}: violation ratio {r}"
        worst["lp"] = r
        s, lp_ref = out["sum"], D["lp"][:B]
        if B == 0:
            assert s == 0.0
        assert abs(s - float(np.sum(out["lp"].astype(np.float64)))) <= 1e-9 * 10 * B, (B, s)
        assert abs(s - float(np.sum(lp_ref))) <= 1e-5 * float(np.sum(np.abs(lp_ref))), (B, s)
        return worst


def _bitwise(a, b, B, what):
    for k, v in a.items():
        if k == "sum":
            continue
        w = b[k][..., :B]
        assert v.shape == w.shape and np.array_equal(v.view(np.int32), w.view(np.int32)), \
            f"{what}: {k} differs bitwise at B = {B}"


def _launches(capfd):
    import torch

    torch.cuda.synchronize()
    return [(m.group(3), int(m.group(4)), int(m.group(5))) for m in LAUNCH.finditer(capfd.readouterr().err)]


@pytest.mark.parametrize("name,choice", _params())
def test_batch_edges(cuda, name, choice, monkeypatch, capfd):
    _, d, n, _, kernel_ids, group, max_tiles = E.CASES[name]
    wide = name in E.WIDE
    forced = {"auto": 0, "t4": 4, "max": max_tiles}[choice]
    H = _Handle(name, forced, monkeypatch, cuda)
    kid = H.h.info.kernel
    assert kid in kernel_ids, f"{name} planned kernel {kid}, expected one of {kernel_ids}"
    kname = E.KERNEL_NAME[kid]
    tiles = 1 if wide else (forced or group)       # wide: reported as kWideT, S is fixed
    S = 128 if wide else 128 * tiles
    pad = 2 * S + 7
    Bmax = 2 * S + 33
    assert Bmax <= H.D["B"]

    capfd.readouterr()
    full = H.run(Bmax, pad)
    seen = _launches(capfd)
    assert len(seen) == 8, seen
    for nm, t, mx in seen:
        assert nm == kname, f"{name}: launched {nm}, expected {kname}"
        if not wide:
            assert mx == max_tiles, f"{name}: the plan's largest tile count is {mx}, the case table says {max_tiles}"
            assert t == tiles, f"{name}: ran {t} tiles per wave, expected {tiles} (DF_TILES={forced or 'unset'})"
    worst = H.check_values(full, Bmax)
    report = (f"EDGE {name} {choice}: kernel {kid} ({kname}) tiles {tiles} max {max_tiles} worst ratio "
              + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))

    for B in (0, 1, 17, S - 1, S, S + 1, S + 16):
        out = H.run(B, pad)
        H.check_values(out, B)
        _bitwise(out, full, B, f"{name} {choice} prefix")
        for nm, t, mx in _launches(capfd):
            assert nm == kname and (wide or t == tiles), (B, nm, t)

    if forced:      # the same batch on the unforced plan of the same chain
        ref = _Handle(name, 0, monkeypatch, cuda)
        capfd.readouterr()
        base = ref.run(Bmax, pad)
        seen = _launches(capfd)
        assert seen and all(nm == kname and t == group for nm, t, mx in seen), seen
        _bitwise(full, base, Bmax, f"{name} DF_TILES={forced} against the unforced plan")
        # the fp64 sum adds one partial per workgroup: its grouping follows S
        assert abs(full["sum"] - base["sum"]) <= 1e-9 * 10 * Bmax
    print(report)       # (after the last capfd read, which would swallow it)


@pytest.mark.parametrize("name", list(E.NORM_ONLY))
def test_normalization_only_chain(cuda, name, monkeypatch, capfd):
    """FlowChain(NormalizationLayer): a plan with no conditioner, no stage and no tables
    (build_plan's `P.stages.empty()` branch).  It runs on the FAST kernel with an empty
    stage schedule; d = 12 takes the element-by-element copy-in with the bounds read from
    global memory.  (The small-batch kernel would load net fragments the 16-byte blob of
    such a chain does not have: use_small() leaves it out.)"""
    H = _Handle(name, 0, monkeypatch, cuda)
    assert H.h.info.kernel == 3 and H.h.info.n_stages == 0
    capfd.readouterr()
    full = H.run(129, 263)
    H.check_values(full, 129)
    for B in (1, 17):
        out = H.run(B, 263)
        H.check_values(out, B)
        _bitwise(out, full, B, f"{name} prefix")
    seen = _launches(capfd)
    assert len(seen) == 24 and all(nm == "uniform-fast" for nm, t, mx in seen), seen
