"""Grid logpdf on the device (df_flow_logpdf_grid, flows.logpdf_grid, logpdf / pdf with x a
tuple of vectors — src/Flows.jl:287-331,345-349).

A chain-pass kernel's output for a sample does not depend on where the sample sits in the
batch (test_gpu_batch_edges.py holds that bitwise), and the generator copies axis values
without arithmetic, so every comparison with the materialised call is BITWISE: a grid
evaluated in chunks equals HIPChain.logpdf on the points the numpy enumerator
(grid_cases.grid_points, pinned in test_grid_host.py) lays out on the host.  Values are held
to the fp64 oracle under close(·, 1e-5) as everywhere else (test_grid_host.py keeps the
oracle's own fp32 below a ratio of 0.5 on these grids).  Output buffers are 64 values longer
than the window and pre-filled with one NaN bit pattern that must survive.
"""
import re

import numpy as np
import pytest

import densityflows_amd as dfa
import edge_cases as E
import grid_cases as G
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from helpers import close, spec_to_element

pytestmark = pytest.mark.gpu

RTOL = 1e-5
NAN32 = 0x7FC0DEAD
PAD = 64
ENV_KEYS = ("DF_TILES", "DF_SMALL_MAX", "DF_SMALL_WAVES", "DF_F32_EXACT", "DF_NO_WIDE", "DF_FORCE_GENERIC",
            "DF_NO_FAST", "DF_NO_FOLD", "DF_DEBUG_LAUNCH")
LAUNCH = re.compile(r"\[df\] mode (\d+) batch (\d+) kernel (\S+) tiles")


def _flat(a, dev):
    """numpy (rows, B) → flat device buffer in Julia memory order (sample-major)."""
    import torch

    return torch.from_numpy(np.array(np.asarray(a, np.float32).T, order="C").ravel()).to(dev)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: differs bitwise"


class _Case:
    """A fresh df_chain of an edge case (its environment read at creation) and the raw calls."""

    def __init__(self, name, monkeypatch, cuda):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        entry = E.CASES.get(name)                      # README16 / norm-only: no environment
        for k, v in (entry[3] if entry else {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
        self.name, self.dev = name, cuda
        self.D = D = E.case_data(G.edge_name(name))
        self.d, self.n = D["d"], D["n"]
        self.model = spec_to_element(D["spec"])
        self.h = self.model.hip(n_hint=self.n)         # the handle Flow.hip() finds in the model's cache
        if self.n:
            self.h.set_theta_bounds(D["tmin"], D["tmax"])
        ids = entry[4] if entry else (3,)
        assert self.h.info.kernel in ids, f"{name} planned kernel {self.h.info.kernel}, expected one of {ids}"
        self.kname = "small" if name == G.README16 else E.KERNEL_NAME[self.h.info.kernel]

    def flow(self):
        """The Flow over the same (cached) handle."""
        D = self.D
        return dfa.Flow(self.model, metadata=MetaData("", self.d, self.n, np.array(D["tmin"]), np.array(D["tmax"])))

    def axes_buf(self, g):
        import torch

        return torch.from_numpy(np.concatenate(g["x_axes"] + g["th_axes"])).to(self.dev)

    def grid(self, g, first, count, chunk, lens=None, axes=None):
        """df_flow_logpdf_grid into a guarded buffer → the count values (pad checked)."""
        import torch

        out = torch.full((count + PAD,), NAN32, dtype=torch.int32, device=self.dev).view(torch.float32)
        self.h.run_logpdf_grid(self.axes_buf(g) if axes is None else axes, g["lens"] if lens is None else lens,
                               first, count, out, chunk)
        torch.cuda.synchronize()
        raw = out.view(torch.int32).cpu().numpy()
        assert np.all(raw[count:] == NAN32), f"{self.name}: written past the window of {count} values"
        return raw[:count].view(np.float32).copy()

    def materialised(self, g):
        """df_flow_logpdf on the host-materialised points of the grid (window)."""
        import torch

        B = g["x"].shape[1]
        lp = torch.empty(B, dtype=torch.float32, device=self.dev)
        self.h.run_logpdf(_flat(g["x"], self.dev), _flat(g["th_raw"], self.dev) if self.n else None, lp, B)
        torch.cuda.synchronize()
        return lp.cpu().numpy()


def _kernels(capfd):
    return [m.group(3) for m in LAUNCH.finditer(capfd.readouterr().err)]


def _check_grid(C, g, capfd, what):
    P = g["x"].shape[1]
    want = C.materialised(g)
    assert np.all(np.isfinite(want))
    ok, r = close(want, g["lp"], RTOL)
    assert ok, f"{what}: materialised logpdf against the fp64 oracle, violation ratio {r}"
    capfd.readouterr()
    for chunk in (0, 64):
        got = C.grid(g, 0, P, chunk)
        seen = _kernels(capfd)
        assert len(seen) == (1 if chunk == 0 else (P + 63) // 64), (chunk, seen)
        assert all(k == C.kname for k in seen), f"{what}: launched {set(seen)}, expected {C.kname}"
        _same_bits(got, want, f"{what} chunk {chunk}")
        ok, r = close(got, g["lp"], RTOL)
        assert ok, f"{what} chunk {chunk}: violation ratio {r}"
    return r


@pytest.mark.parametrize("name", G.BITWISE_CASES)
def test_grid_is_bitwise_the_materialised_call(cuda, name, monkeypatch, capfd):
    C = _Case(name, monkeypatch, cuda)
    g = G.grid_data(name, G.LENS_X[C.d])
    assert 144 <= g["x"].shape[1] <= 420
    r = _check_grid(C, g, capfd, name)
    if name == "split64":
        many = G.grid_data(name, G.LENS_MANY)
        assert many["x"].shape[1] == 1260
        r = max(r, _check_grid(C, many, capfd, f"{name} 1260 points"))
    print(f"GRID {name}: kernel {C.kname}, worst violation ratio {r:.3f}")


def test_windows_concatenate_to_the_full_grid(cuda, monkeypatch):
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", G.LENS5)
    P = g["x"].shape[1]
    full = C.grid(g, 0, P, 0)
    parts = [C.grid(g, a, b - a, chunk) for (a, b), chunk in zip(((0, 100), (100, 163), (163, P)), (0, 64, 0))]
    assert all(a % 64 for a in (100, 163))
    _same_bits(np.concatenate(parts), full, "windows [0,100) [100,163) [163,P)")
    _same_bits(full, C.materialised(g), "full grid")


def test_window_past_2_33(cuda, monkeypatch):
    """P = 2³⁵: the point number needs 64 bits, only the window is evaluated."""
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", (G.BIG_LEN,) * 5, None, G.BIG_FIRST, G.BIG_COUNT)
    assert int(np.prod(g["lens"], dtype=np.int64)) == 2**35
    want = C.materialised(g)
    for chunk in (0, 64):
        got = C.grid(g, G.BIG_FIRST, G.BIG_COUNT, chunk)
        _same_bits(got, want, f"window at 2^33 + 5, chunk {chunk}")
        ok, r = close(got, g["lp"], RTOL)
        assert ok, r
    via_api = dfa.logpdf_grid(C.flow(), tuple(g["x_axes"]), tuple(g["th_axes"]), first=G.BIG_FIRST,
                              count=G.BIG_COUNT)
    assert isinstance(via_api, np.ndarray) and via_api.shape == (G.BIG_COUNT,)
    _same_bits(via_api, want, "logpdf_grid window")


def test_strides_past_32_bits(cuda, monkeypatch):
    """Axes of 65536 values put the strides of the last three axes at 2³², 3·2³² and 6·2³²;
    all three step inside the window."""
    C = _Case("split64", monkeypatch, cuda)
    g = G.grid_data("split64", G.HUGE_LENS, None, G.HUGE_FIRST, G.BIG_COUNT)
    assert len({tuple(c) for c in g["x"][2:].T}) == 2 and np.all(g["x"][2:, 0] != g["x"][2:, -1])
    want = C.materialised(g)
    for chunk in (0, 64):
        got = C.grid(g, G.HUGE_FIRST, G.BIG_COUNT, chunk)
        _same_bits(got, want, f"strides past 2^32, chunk {chunk}")
        ok, r = close(got, g["lp"], RTOL)
        assert ok, r


@pytest.mark.parametrize("name", list(G.THETA_AXES))
def test_theta_axes(cuda, name, monkeypatch):
    """A likelihood surface: θ entries given as vectors are grid axes after the x axes."""
    C = _Case(name, monkeypatch, cuda)
    g = G.grid_data(name, G.LENS_X[C.d], G.THETA_AXES[name])
    want = C.materialised(g)
    for chunk in (0, 64):
        _same_bits(C.grid(g, 0, want.size, chunk), want, f"{name} θ axes, chunk {chunk}")
    # a θ entry of length 1 as a plain value, the other as a vector
    th = tuple(float(a[0]) if a.size == 1 else a for a in g["th_axes"])
    res = dfa.logpdf_grid(C.flow(), tuple(g["x_axes"]), th, chunk=64)
    assert isinstance(res, np.ndarray) and res.shape == G.LENS_X[C.d] + G.THETA_AXES[name] == g["lens"]
    _same_bits(res.reshape(-1, order="F"), want, f"{name} logpdf_grid")
    ok, r = close(res.reshape(-1, order="F"), g["lp"], RTOL)
    assert ok, r


def test_public_api(cuda, monkeypatch):
    import torch

    C = _Case("split64", monkeypatch, cuda)
    flow, g = C.flow(), dict(G.grid_data("split64", G.LENS5))
    g["x"], g["th_raw"] = np.array(g["x"]), np.array(g["th_raw"])      # writable copies for torch.from_numpy
    axes, th = tuple(g["x_axes"]), tuple(float(a[0]) for a in g["th_axes"])
    res = dfa.logpdf(flow, axes, th)
    assert isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == G.LENS5
    by_array = dfa.logpdf(flow, g["x"], g["th_raw"])
    assert by_array.shape == (g["x"].shape[1],)
    _same_bits(res, by_array.reshape(G.LENS5, order="F"), "logpdf(flow, axes, θ)")
    ok, r = close(res.reshape(-1, order="F"), g["lp"], RTOL)
    assert ok, r
    _same_bits(dfa.pdf(flow, axes, th), np.exp(res), "pdf(flow, axes, θ)")
    # device tensors in, a device tensor out, the same values
    dres = dfa.logpdf(flow, tuple(torch.from_numpy(np.array(a)).to(cuda) for a in axes), th)
    assert isinstance(dres, torch.Tensor) and dres.device.type == "cuda" and tuple(dres.shape) == G.LENS5
    _same_bits(dres.cpu().numpy(), res, "device axes")
    # array x with an NTuple θ: bitwise the explicit (n, P) array, on the device all the way
    _same_bits(dfa.logpdf(flow, g["x"], th), by_array, "array logpdf, NTuple θ")
    _same_bits(dfa.pdf(flow, g["x"], th), np.exp(by_array), "array pdf, NTuple θ")
    s1, b1 = dfa.nll_partial_sum(flow, g["x"], th)
    s2, b2 = dfa.nll_partial_sum(flow, g["x"], g["th_raw"])
    assert b1 == b2 and s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    x3 = g["x"][:, :30].reshape(5, 5, 6, order="F")
    _same_bits(dfa.logpdf(flow, x3, th), by_array[:30].reshape(5, 6, order="F"), "array logpdf (d, 5, 6), NTuple θ")
    # the reference's two shape errors (Flows.jl:247-249 and the NTuple{D} dispatch)
    with pytest.raises(_lib.DimensionMismatch):
        dfa.logpdf(flow, axes, g["th_raw"])
    with pytest.raises(_lib.DimensionMismatch):
        dfa.logpdf(flow, axes[:4], th)
    with pytest.raises(_lib.DimensionMismatch):
        dfa.logpdf(flow, axes, th + (0.5,))


def test_public_api_unconditional(cuda, monkeypatch):
    C = _Case("norm_only_d5", monkeypatch, cuda)
    flow, g = C.flow(), G.grid_data("norm_only_d5", G.LENS5)
    axes = tuple(g["x_axes"])
    res = dfa.logpdf(flow, axes)
    assert isinstance(res, np.ndarray) and res.shape == G.LENS5
    _same_bits(res, dfa.logpdf(flow, g["x"]).reshape(G.LENS5, order="F"), "logpdf(flow, axes)")
    _same_bits(dfa.pdf(flow, axes), np.exp(res), "pdf(flow, axes)")
    _same_bits(dfa.logpdf_grid(flow, axes), res, "logpdf_grid(flow, axes)")
    ok, r = close(res.reshape(-1, order="F"), g["lp"], RTOL)
    assert ok, r
    with pytest.raises(_lib.DimensionMismatch):
        dfa.logpdf(flow, axes + (axes[0],))


def test_edges_and_handle_state(cuda, monkeypatch, capfd):
    import torch

    C = _Case("split64", monkeypatch, cuda)
    flow, g = C.flow(), G.grid_data("split64", G.LENS5)
    P, h = g["x"].shape[1], C.h
    xb, tb = _flat(g["x"], cuda), _flat(g["th_raw"], cuda)
    th = tuple(float(a[0]) for a in g["th_axes"])

    def state():
        lp = torch.empty(P, dtype=torch.float32, device=cuda)
        h.run_logpdf(xb, tb, lp, P)
        smp = dfa.sample(flow, (3, 50), th, seed=12345, offset=7)
        torch.cuda.synchronize()
        return lp.cpu().numpy(), smp.cpu().numpy()

    lp0, smp0 = state()
    capfd.readouterr()
    # nothing to do: OK, no launch, output untouched (the guard of C.grid covers all of it)
    assert C.grid(g, 0, 0, 0).size == 0 and C.grid(g, P, 0, 64).size == 0
    lens0 = list(g["lens"])
    lens0[2] = 0
    axes0 = torch.from_numpy(np.concatenate([a for k, a in enumerate(g["x_axes"] + g["th_axes"]) if k != 2])).to(cuda)
    assert C.grid(g, 0, 0, 0, lens=lens0, axes=axes0).size == 0
    assert _kernels(capfd) == []
    empty = dfa.logpdf_grid(flow, tuple(a if k != 2 else a[:0] for k, a in enumerate(g["x_axes"])), th)
    assert empty.shape == (3, 1, 0, 2, 7, 1)
    # windows outside the grid, a negative length, a wrong number of lengths
    room = torch.empty(P + PAD, dtype=torch.float32, device=cuda)
    for first, count in ((0, P + 1), (P, 1), (-1, 2), (0, -1), (1, 2**63 - 1)):      # the last: first + count wraps
        with pytest.raises(_lib.DimensionMismatch):
            h.run_logpdf_grid(C.axes_buf(g), g["lens"], first, count, room, 0)
    with pytest.raises(_lib.DimensionMismatch):
        C.grid(g, 0, 1, 0, lens=[3, 1, -5, 2, 7, 1])
    with pytest.raises(_lib.DimensionMismatch):
        C.grid(g, 0, 1, 0, lens=[2**31] * 5 + [1])         # P past int64
    with pytest.raises(_lib.DimensionMismatch):
        C.grid(g, 0, 1, 0, lens=list(g["lens"][:-1]))
    with pytest.raises(_lib.DimensionMismatch):
        dfa.logpdf_grid(flow, tuple(g["x_axes"]), th, first=P - 3, count=4)
    with pytest.raises(_lib.ArgumentError):
        h.run_logpdf_grid(None, g["lens"], 0, 1, torch.empty(1, device=cuda), 0)   # null axes
    assert _kernels(capfd) == []
    # a grid call (staging grown twice) leaves the handle's other entry points as they were
    C.grid(g, 0, P, 64)
    C.grid(g, 0, P, 0)
    lp1, smp1 = state()
    _same_bits(lp1, lp0, "logpdf after a grid call")
    _same_bits(smp1, smp0, "sample after a grid call")
