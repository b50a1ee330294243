"""HIP executor: compiles a flow element into a ``df_chain`` handle and runs
the fused kernels on device arrays.

Array convention (mirrors the reference): a batch is an array of logical
shape ``(d, dims...)`` in Julia memory order (column-major: each sample's d
values are contiguous).  torch tensors whose *reversed-axes view* is
contiguous are used zero-copy; anything else (numpy arrays, other strides) is
copied once into that layout.  Outputs are returned with the same logical
shape, as column-major views of a fresh contiguous buffer.

PyTorch is used only as plumbing (device allocation, streams).  There is no
CPU fallback: without the native library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _lib
from .layers import (CouplingBlock, NICECouplingLayer, NormalizationLayer, RNVPCouplingLayer)

__all__ = ["HIPChain", "flatten_elements", "as_julia_device", "julia_empty", "chain_dims", "run_order_statistics",
           "run_draw_histograms", "run_importance_weights", "run_draw_weighted_stats", "run_draw_resample",
           "run_draw_weight_scale", "run_draw_weighted_quantiles", "run_draw_weighted_histograms"]


def _torch():
    import torch  # plumbing only

    return torch


# ---------------------------------------------------------------------------
# layout helpers
# ---------------------------------------------------------------------------

def julia_empty(rows: int, dims: Tuple[int, ...], device):
    """A column-major (rows, dims...) float32 tensor: returns (flat buffer, logical view)."""
    torch = _torch()
    shape_rev = tuple(reversed(dims)) + (rows,)
    buf = torch.empty(shape_rev, dtype=torch.float32, device=device)
    nd = len(shape_rev)
    view = buf.permute(*reversed(range(nd)))
    return buf.reshape(-1), view


def as_julia_device(a, rows: int, device, name: str = "array"):
    """Return (flat contiguous device buffer in Julia order, dims, was_numpy)."""
    torch = _torch()
    was_numpy = not isinstance(a, torch.Tensor)
    if was_numpy:
        a = np.asarray(a, dtype=np.float32)
        if a.ndim < 1 or a.shape[0] != rows:
            raise _lib.DimensionMismatch(f"{name} must have size ({rows}, dims...), got {a.shape}")
        # Julia memory order = Fortran order of the logical array
        host = np.asfortranarray(a).ravel(order="K")
        t = torch.from_numpy(np.ascontiguousarray(host)).to(device)
        return t, tuple(a.shape[1:]), True
    if a.dtype != torch.float32:
        raise _lib.ArgumentError(f"{name} must be Float32 (got {a.dtype})")
    if a.dim() < 1 or a.shape[0] != rows:
        raise _lib.DimensionMismatch(f"{name} must have size ({rows}, dims...), got {tuple(a.shape)}")
    if a.device.type != "cuda":
        a = a.to(device)
    rev = a.permute(*reversed(range(a.dim())))
    if not rev.is_contiguous():
        rev = rev.contiguous()
    return rev.reshape(-1), tuple(a.shape[1:]), was_numpy


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else C.c_void_p(0)


def _stream(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---------------------------------------------------------------------------
# descriptor construction
# ---------------------------------------------------------------------------

def flatten_elements(elements) -> List[Tuple[int, object]]:
    """Flatten a chain into (element index, layer) pairs.

    CouplingBlocks give two layers with one element index (ldj_1 .+ ldj_2,
    src/Blocks.jl:136,149); a nested FlowChain is flattened into one element
    (its inner ldj is accumulated left to right, equal to the reference up to
    fp32 summation order when it contains blocks)."""
    from .chains import FlowChain

    out = []
    for e_idx, e in enumerate(elements):
        if isinstance(e, CouplingBlock):
            out += [(e_idx, e.layer_1), (e_idx, e.layer_2)]
        elif isinstance(e, FlowChain):
            for _, l in flatten_elements(e.layers):
                out.append((e_idx, l))
        elif isinstance(e, (RNVPCouplingLayer, NICECouplingLayer, NormalizationLayer)):
            out.append((e_idx, e))
        else:
            raise _lib.UnsupportedError(f"no fused kernel for flow element {type(e).__name__}")
    return out


def chain_dims(flat, n_hint: int | None = None) -> Tuple[int, int]:
    d = n = None
    for _, l in flat:
        if isinstance(l, NormalizationLayer):
            dd = l.x_min.shape[0]
            if d is not None and dd != d:
                raise _lib.DimensionMismatch("NormalizationLayer dimension does not match the chain")
            d = dd
        else:
            if d is not None and l.axes.d != d:
                raise _lib.DimensionMismatch("layers of a chain must share the dimension d")
            if n is not None and l.axes.n != n:
                raise _lib.DimensionMismatch("layers of a chain must share the number of conditions n")
            d, n = l.axes.d, l.axes.n
    if n is None:
        n = n_hint or 0
    return d, n


class _Desc:
    """Owns the ctypes descriptor and every host array it points to."""

    def __init__(self, flat, d, n):
        self.keep = []
        layers = (_lib.df_layer_desc * len(flat))()
        for i, (e_idx, l) in enumerate(flat):
            L = layers[i]
            L.element = e_idx
            if isinstance(l, NormalizationLayer):
                L.kind = _lib.DF_LAYER_NORM
                L.x_min = self._fp(l.x_min)
                L.x_max = self._fp(l.x_max)
                L.alpha = l.alpha
                L.beta = l.beta
                continue
            L.kind = _lib.DF_LAYER_RNVP if isinstance(l, RNVPCouplingLayer) else _lib.DF_LAYER_NICE
            L.n_af = len(l.axes.axis_af)
            L.axis_af = self._ip(l.axes.axis_af)
            L.n_nn = len(l.axes.axis_nn)
            L.axis_nn = self._ip(l.axes.axis_nn)
            if isinstance(l, RNVPCouplingLayer):
                L.n_dense_s, L.s_net = self._net(l.s_net)
            L.n_dense_t, L.t_net = self._net(l.t_net)
        self.keep.append(layers)
        self.desc = _lib.df_chain_desc(_lib.ABI_VERSION, d, n, len(flat), layers)

    def _fp(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        self.keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_float))

    def _ip(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        self.keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def _net(self, net):
        arr = (_lib.df_dense_desc * len(net))()
        for k, D in enumerate(net):
            W = np.asfortranarray(D.W, dtype=np.float32)  # Flux column-major (out, in)
            self.keep.append(W)
            arr[k].in_dim = D.in_dim
            arr[k].out_dim = D.out_dim
            arr[k].act = _lib.ACTIVATIONS[D.act]
            arr[k].W = W.ctypes.data_as(C.POINTER(C.c_float))
            arr[k].b = self._fp(D.b) if D.b is not None else C.POINTER(C.c_float)()
        self.keep.append(arr)
        return len(net), arr


def validate(elements, n_hint: int | None = None):
    """Host-only planning (no device): returns df_chain_info or raises."""
    lib = _lib.load()
    flat = flatten_elements(elements)
    d, n = chain_dims(flat, n_hint)
    desc = _Desc(flat, d, n)
    info = _lib.df_chain_info()
    _lib.check(lib.df_chain_validate(C.byref(desc.desc), C.byref(info)), "df_chain_validate")
    return info


def _orders_array(orders):
    """(ctypes int32 array or None, count) of host integers."""
    if orders is None:
        return None, 0
    vals = [int(v) for v in orders]
    return (C.c_int32 * max(len(vals), 1))(*vals), len(vals)


def run_order_statistics(xs, d: int, n_points: int, n_draws: int, orders, out):
    """df_order_statistics: the order statistics ``orders`` (host integers in ``[0, n_draws)``) of
    every dimension of the ``n_points`` points of the device tensor ``xs`` (d, n_points · n_draws;
    draw j of point i at ``d·(i·n_draws + j)``, 16-byte aligned) into the float32 device tensor
    ``out``, element ``(i·d + k)·len(orders) + q``, on ``xs``' device and its current stream."""
    import torch

    arr, nq = _orders_array(orders)
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        _lib.check(lib.df_order_statistics(_ptr(xs), C.c_int(d), C.c_int64(n_points), C.c_int64(n_draws), arr,
                                           C.c_int(nq), _ptr(out), _stream(xs.device)), "order_statistics")


def _tables_arrays(bins, keep):
    """(ctypes int32 bins or None, ctypes int32 requests or None, table count) of host integers:
    ``keep`` holds one tuple ``(a,)`` or ``(a, b)`` per table."""
    if bins is None or keep is None:
        return None, None, 0
    b = [int(v) for v in bins]
    flat = [int(v) for k in keep for v in (tuple(k) + (-1,))[:2]]
    return (C.c_int32 * max(len(b), 1))(*b), (C.c_int32 * max(len(flat), 2))(*flat), len(keep)


def run_draw_histograms(xs, d: int, n_points: int, n_draws: int, edges, bins, keep, counts):
    """df_draw_histograms: the 1-D and 2-D tables ``keep`` (host tuples ``(a,)`` / ``(a, b)``,
    a < b) of the ``n_points`` points of the device tensor ``xs`` (d, n_points · n_draws; draw j of
    point i at ``d·(i·n_draws + j)``, 16-byte aligned) into the int32 device tensor ``counts``:
    per point a block of the tables in request order, index ``i_a + L_a·i_b``.  ``bins``: d host
    integers; ``edges``: float32 device tensor, the ``bins[k] + 1`` edges of every dimension with
    bins, one after the other.  On ``xs``' device and its current stream."""
    import torch

    barr, karr, nt = _tables_arrays(bins, keep)
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        _lib.check(lib.df_draw_histograms(_ptr(xs), C.c_int(d), C.c_int64(n_points), C.c_int64(n_draws), _ptr(edges),
                                          barr, karr, C.c_int32(nt), _ptr(counts), _stream(xs.device)),
                   "draw_histograms")


def run_importance_weights(logw, n_points: int, n_draws: int, w=None, stats=None):
    """df_importance_weights: the float32 device tensor ``logw`` (n_points · n_draws, draw j of
    point i at ``i·n_draws + j``, 16-byte aligned) into the stabilised weights
    ``expf(logw − max)`` (float32 device tensor ``w``, not overlapping ``logw``) and, per point, the
    four float64 ``{max, Σ w, Σ w², #{w > 0}}`` of the device tensor ``stats``; at least one of
    the two.  On ``logw``'s device and its current stream."""
    import torch

    lib = _lib.load()
    with torch.cuda.device(logw.device):
        _lib.check(lib.df_importance_weights(_ptr(logw), C.c_int64(n_points), C.c_int64(n_draws), _ptr(w),
                                             _ptr(stats), _stream(logw.device)), "importance_weights")


def run_draw_weighted_stats(xs, w, x, d: int, n_points: int, n_draws: int, wrank=None, sums=None):
    """df_draw_weighted_stats: the ``n_points`` points of the device tensor ``xs`` (d, n_points ·
    n_draws; draw j of point i at ``d·(i·n_draws + j)``) under the float32 weights ``w`` (n_points ·
    n_draws), both 16-byte aligned, reduced per point.  ``wrank`` (float64, d · n_points; needs the
    points ``x`` (d, n_points)) takes ``Σ w·[draw[k] < x[k]]``, ``sums`` (float64, n_points blocks of
    2 + 2d + d(d+1)/2) ``Σ w``, ``Σ w²``, the shift, ``Σ w·(draw − c)`` and the lower triangle of
    ``Σ w·(draw − c)(draw − c)ᵀ``; at least one of the two.  On ``xs``' device and its current
    stream."""
    import torch

    lib = _lib.load()
    with torch.cuda.device(xs.device):
        _lib.check(lib.df_draw_weighted_stats(_ptr(xs), _ptr(w), _ptr(x), C.c_int(d), C.c_int64(n_points),
                                              C.c_int64(n_draws), _ptr(wrank), _ptr(sums), _stream(xs.device)),
                   "draw_weighted_stats")


def run_draw_resample(xs, w, d: int, n_points: int, n_draws: int, n_out: int, method: int, seed: int, offset: int,
                      xs_out=None, idx_out=None, cdf_ws=None):
    """df_draw_resample: per point ``n_out`` picks among the ``n_draws`` draws of the float32 device
    tensor ``w`` (n_points · n_draws, 16-byte aligned) by ``method`` (0 systematic, 1 stratified,
    2 multinomial) from the Philox stream ``(seed, offset)``: the indices within the point (or −1)
    into the int32 device tensor ``idx_out`` (n_points · n_out) and the picked rows of ``xs``
    (d, n_points · n_draws; 16-byte aligned) into ``xs_out`` (d, n_points · n_out), which must not
    overlap ``xs``; at least one of the two, and without ``xs_out`` neither ``xs`` nor ``d`` is
    looked at.  ``cdf_ws``: a device tensor of n_points · n_draws 8-byte words, needed above 4096
    draws.  On ``w``'s device and its current stream."""
    import torch

    lib = _lib.load()
    with torch.cuda.device(w.device):
        _lib.check(lib.df_draw_resample(_ptr(xs), _ptr(w), _ptr(cdf_ws), C.c_int(d), C.c_int64(n_points),
                                        C.c_int64(n_draws), C.c_int64(n_out), C.c_int(method),
                                        C.c_uint64(seed), C.c_uint64(offset), _ptr(xs_out), _ptr(idx_out), _stream(w.device)), "draw_resample")


def run_draw_weight_scale(w, n_points: int, n_draws: int, scale):
    """df_draw_weight_scale: per point of the float32 device tensor ``w`` (n_points · n_draws, 16-byte
    aligned) the two int64 ``{e, T}`` of the device tensor ``scale`` — the exponent of its largest
    weight that takes part and the sum of its quantised weights, ``{0, 0}`` for an empty point.  On
    ``w``'s device and its current stream."""
    import torch

    lib = _lib.load()
    with torch.cuda.device(w.device):
        _lib.check(lib.df_draw_weight_scale(_ptr(w), C.c_int64(n_points), C.c_int64(n_draws), _ptr(scale),
                                            _stream(w.device)), "draw_weight_scale")


def run_draw_weighted_quantiles(xs, w, d: int, n_points: int, n_draws: int, nums, out, scale):
    """df_draw_weighted_quantiles: the weighted quantiles at the numerators ``nums`` (host integers in
    ``[0, 2^32]`` over the denominator 2^32) of every dimension of the ``n_points`` points of the
    device tensor ``xs`` (d, n_points · n_draws) under the float32 weights ``w`` (n_points · n_draws),
    both 16-byte aligned, into the float32 device tensor ``out``, element
    ``(i·d + k)·len(nums) + q``; ``scale`` (int64, 2 per point) takes ``{e, T}``.  On ``xs``' device
    and its current stream."""
    import torch

    vals = [int(v) for v in nums]
    arr = (C.c_uint64 * max(len(vals), 1))(*vals)
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        _lib.check(lib.df_draw_weighted_quantiles(_ptr(xs), _ptr(w), C.c_int(d), C.c_int64(n_points),
                                                  C.c_int64(n_draws), arr, C.c_int(len(vals)), _ptr(out), _ptr(scale),
                                                  _stream(xs.device)), "draw_weighted_quantiles")


def run_draw_weighted_histograms(xs, w, d: int, n_points: int, n_draws: int, edges, bins, keep, sums, scale):
    """df_draw_weighted_histograms: the tables ``keep`` of :func:`run_draw_histograms` (``edges``,
    ``bins`` as there) with, per bin, the sum of the quantised weights of its draws: ``sums`` is an
    int64 device tensor whose words hold the uint64 sums, per point a block of the tables in request
    order; ``w`` the float32 weights (n_points · n_draws, 16-byte aligned); ``scale`` (int64, 2 per
    point) takes ``{e, T}``.  On ``xs``' device and its current stream."""
    import torch

    barr, karr, nt = _tables_arrays(bins, keep)
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        _lib.check(lib.df_draw_weighted_histograms(_ptr(xs), _ptr(w), C.c_int(d), C.c_int64(n_points),
                                                   C.c_int64(n_draws), _ptr(edges), barr, karr, C.c_int32(nt),
                                                   _ptr(sums), _ptr(scale), _stream(xs.device)),
                   "draw_weighted_histograms")


class HIPChain:
    """A device-resident compiled chain (one ``df_chain`` handle per device)."""

    def __init__(self, elements, device=None, n_hint: int | None = None):
        torch = _torch()
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HIPError("no HIP device visible: the fused kernels need an MI355X (gfx950)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        flat = flatten_elements(elements)
        self.d, self.n = chain_dims(flat, n_hint)
        desc = _Desc(flat, self.d, self.n)
        h = C.c_void_p()
        _lib.check(self.lib.df_chain_create(C.byref(h), C.byref(desc.desc), self.device.index), "df_chain_create")
        self.handle = h
        self.info = _lib.df_chain_info()
        _lib.check(self.lib.df_chain_get_info(self.handle, C.byref(self.info)))
        self.bounds = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.df_chain_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self.handle = None

    def set_weights(self, elements) -> None:
        """df_chain_set_weights: take the parameters of ``elements`` (same structure)."""
        flat = flatten_elements(elements)
        d, n = chain_dims(flat, self.n)
        if (d, n) != (self.d, self.n):
            raise _lib.DimensionMismatch("set_weights: (d, n) differ from the chain's")
        desc = _Desc(flat, d, n)
        _lib.check(self.lib.df_chain_set_weights(self.handle, C.byref(desc.desc)), "df_chain_set_weights")

    def set_theta_bounds(self, tmin, tmax):
        tmin = np.ascontiguousarray(tmin, dtype=np.float32).reshape(-1)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
        if tmin.shape[0] != self.n or tmax.shape[0] != self.n:
            raise _lib.DimensionMismatch("θ bounds must have n entries")
        _lib.check(self.lib.df_chain_set_theta_bounds(
            self.handle, tmin.ctypes.data_as(C.POINTER(C.c_float)), tmax.ctypes.data_as(C.POINTER(C.c_float))))
        self.bounds = (tmin.copy(), tmax.copy())

    # -- diagnostics ---------------------------------------------------------
    def clock_probe(self, on: bool = True) -> None:
        """df_chain_clock_probe: stamp the effective shader clock of later passes."""
        _lib.check(self.lib.df_chain_clock_probe(self.handle, 1 if on else 0), "df_chain_clock_probe")

    def clock_read(self):
        """df_chain_clock_read → (median GHz over workgroup slots, Σcycles/Σtime GHz, slots)."""
        med, mean, slots = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(self.lib.df_chain_clock_read(self.handle, C.byref(med), C.byref(mean), C.byref(slots)),
                   "df_chain_clock_read")
        return med.value, mean.value, slots.value

    # -- raw entry points on flat device buffers ---------------------------
    def run(self, op: str, zbuf, thbuf, outbuf, ldjbuf, batch: int, flow: bool = False):
        fn = {
            ("forward", False): self.lib.df_chain_forward, ("forward", True): self.lib.df_flow_forward,
            ("backward", False): self.lib.df_chain_backward, ("backward", True): self.lib.df_flow_backward,
        }[(op, flow)]
        _lib.check(fn(self.handle, _ptr(zbuf), _ptr(thbuf), _ptr(outbuf), _ptr(ldjbuf), C.c_int64(batch),
                      _stream(self.device)), op)

    def run_inplace(self, zbuf, thbuf, batch: int, flow: bool = False):
        fn = self.lib.df_flow_forward_inplace if flow else self.lib.df_chain_forward_inplace
        _lib.check(fn(self.handle, _ptr(zbuf), _ptr(thbuf), C.c_int64(batch), _stream(self.device)), "forward!")

    def run_logpdf(self, xbuf, thbuf, lpbuf, batch: int):
        _lib.check(self.lib.df_flow_logpdf(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(lpbuf), C.c_int64(batch),
                                           _stream(self.device)), "logpdf")

    def run_logpdf_sum(self, xbuf, thbuf, sumbuf, batch: int):
        _lib.check(self.lib.df_flow_logpdf_sum(self.handle, _ptr(xbuf), _ptr(thbuf),
                                               C.c_void_p(sumbuf.data_ptr()), C.c_int64(batch),
                                               _stream(self.device)), "logpdf_sum")

    def run_logpdf_wsum(self, xbuf, thbuf, wbuf, sumbuf, batch: int):
        """df_flow_logpdf_wsum on flat device buffers: ``{Σ w·logpdf, Σ w}`` into the two
        float64 of ``sumbuf``."""
        _lib.check(self.lib.df_flow_logpdf_wsum(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(wbuf),
                                                C.c_int64(batch), C.c_void_p(sumbuf.data_ptr()),
                                                _stream(self.device)), "logpdf_wsum")

    def run_logpdf_grid(self, axes_buf, lens, first: int, count: int, lpbuf, chunk: int = 0):
        """df_flow_logpdf_grid: logpdf on points [first, first + count) of the outer product of
        the d + n axis vectors concatenated in ``axes_buf`` (first axis fastest), evaluated
        ``chunk`` points at a time (0: the library's default)."""
        if len(lens) != self.d + self.n:
            raise _lib.DimensionMismatch(f"a grid needs d + n = {self.d + self.n} axis lengths, got {len(lens)}")
        arr = (C.c_int64 * max(len(lens), 1))(*[int(v) for v in lens])
        _lib.check(self.lib.df_flow_logpdf_grid(self.handle, _ptr(axes_buf), arr, C.c_int64(first),
                                                C.c_int64(count), _ptr(lpbuf), C.c_int64(chunk),
                                                _stream(self.device)), "logpdf_grid")

    def run_pdf_marginals(self, axes_buf, weights_buf, lens, first: int, count: int, keep, outbuf, chunk: int = 0):
        """df_flow_pdf_marginals: the marginal tables of pdf over points [first, first + count)
        of the grid of ``run_logpdf_grid``, into the float64 device buffer ``outbuf`` one after
        the other.  ``weights_buf``: float64, laid out like ``axes_buf``.  ``keep``: one tuple
        of 0, 1 or 2 ascending axis numbers per table."""
        if len(lens) != self.d + self.n:
            raise _lib.DimensionMismatch(f"a grid needs d + n = {self.d + self.n} axis lengths, got {len(lens)}")
        if any(len(k) > 2 for k in keep):
            raise _lib.UnsupportedError("a marginal keeps at most two axes")
        arr = (C.c_int64 * max(len(lens), 1))(*[int(v) for v in lens])
        flat = [int(v) for k in keep for v in (tuple(k) + (-1, -1))[:2]]
        req = (C.c_int32 * max(len(flat), 1))(*flat)
        _lib.check(self.lib.df_flow_pdf_marginals(self.handle, _ptr(axes_buf), _ptr(weights_buf), arr,
                                                  C.c_int64(first), C.c_int64(count), req, C.c_int32(len(keep)),
                                                  _ptr(outbuf), C.c_int64(chunk), _stream(self.device)),
                   "pdf_marginals")

    def run_theta_broadcast(self, outbuf, thvec, batch: int):
        """df_theta_broadcast: the n-vector ``thvec`` into every column of the (n, batch) ``outbuf``."""
        _lib.check(self.lib.df_theta_broadcast(_ptr(outbuf), _ptr(thvec), C.c_int(int(thvec.numel())),
                                               C.c_int64(batch), _stream(self.device)), "θ broadcast")

    def run_sample(self, xbuf, thbuf, broadcast: bool, batch: int, seed: int, offset: int = 0):
        """df_flow_sample: device N(0, I) draw (Philox, seed/offset) + fused forward!."""
        _lib.check(self.lib.df_flow_sample(self.handle, _ptr(xbuf), _ptr(thbuf), 1 if broadcast else 0,
                                           C.c_int64(batch), C.c_uint64(seed), C.c_uint64(offset),
                                           _stream(self.device)), "sample")

    def run_sample_logpdf(self, xbuf, lpbuf, thbuf, broadcast: bool, batch: int, seed: int, offset: int = 0):
        """df_flow_sample_logpdf: the draw sent through ``forward`` into ``xbuf`` and
        ``log q(x | θ)`` of every drawn point into ``lpbuf`` (None: the draw and forward alone)."""
        _lib.check(self.lib.df_flow_sample_logpdf(self.handle, _ptr(xbuf), _ptr(lpbuf), _ptr(thbuf),
                                                  1 if broadcast else 0, C.c_int64(batch), C.c_uint64(seed),
                                                  C.c_uint64(offset), _stream(self.device)), "sample_logpdf")

    def run_sample_logpdf_moments(self, thvec, n_samples: int, chunk: int, seed: int, offset: int, outbuf):
        """df_flow_sample_logpdf_moments: ``{count, Σ lp, Σ lp²}`` of ``n_samples`` draws at the
        ONE raw θ ``thvec`` (device n-vector, None for n = 0) into the three float64 of ``outbuf``."""
        _lib.check(self.lib.df_flow_sample_logpdf_moments(self.handle, _ptr(thvec), C.c_int64(n_samples),
                                                          C.c_int64(chunk), C.c_uint64(seed), C.c_uint64(offset),
                                                          _ptr(outbuf), _stream(self.device)),
                   "sample_logpdf_moments")

    def run_hpd_ranks(self, xbuf, thbuf, n_points: int, n_draws: int, chunk: int, seed: int, offset: int, rankbuf,
                      lpbuf=None, drawsbuf=None):
        """df_flow_hpd_ranks: for each of the ``n_points`` columns of ``xbuf`` (d, n_points) under
        the raw θ columns of ``thbuf`` (n, n_points), the number of ``n_draws`` draws of the flow
        at that θ whose density exceeds the point's, into the int32 ``rankbuf``.  ``lpbuf``
        (n_points) takes the points' logpdf and ``drawsbuf`` (n_points · n_draws) the draws',
        when given."""
        _lib.check(self.lib.df_flow_hpd_ranks(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(n_points),
                                              C.c_int64(n_draws), C.c_int64(chunk), C.c_uint64(seed),
                                              C.c_uint64(offset), _ptr(rankbuf), _ptr(lpbuf), _ptr(drawsbuf),
                                              _stream(self.device)), "hpd_ranks")

    def run_point_stats(self, xbuf, thbuf, n_points: int, n_draws: int, chunk: int, seed: int, offset: int,
                        rankbuf=None, sumsbuf=None, drawsbuf=None):
        """df_flow_point_stats: ``n_draws`` draws of the flow at each of the ``n_points`` raw θ
        columns of ``thbuf`` (n, n_points), reduced per point.  ``rankbuf`` (int32, d · n_points;
        needs the points ``xbuf`` (d, n_points)) takes the SBC ranks ``#{draw[k] < x[k]}``,
        ``sumsbuf`` (float64, n_points blocks of 2d + d(d+1)/2) the shift, ``Σ (draw − c)`` and the
        lower triangle of ``Σ (draw − c)(draw − c)ᵀ``, ``drawsbuf`` (d · n_points · n_draws) the
        draws themselves; at least one of the three."""
        _lib.check(self.lib.df_flow_point_stats(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(n_points),
                                                C.c_int64(n_draws), C.c_int64(chunk), C.c_uint64(seed),
                                                C.c_uint64(offset), _ptr(rankbuf), _ptr(sumsbuf), _ptr(drawsbuf),
                                                _stream(self.device)), "point_stats")

    def run_point_quantiles(self, xbuf, thbuf, n_points: int, n_draws: int, chunk: int, seed: int, offset: int,
                            orders, quantbuf=None, rankbuf=None, sumsbuf=None, drawsbuf=None):
        """df_flow_point_quantiles: :meth:`run_point_stats` with the selection at the end of every
        chunk.  ``quantbuf`` (float32, d · n_points · len(orders)) takes the order statistics
        ``orders`` (host integers in ``[0, n_draws)``) of every dimension of every point, element
        ``(i·d + k)·len(orders) + q``; ``rankbuf``, ``sumsbuf`` and ``drawsbuf`` as for
        :meth:`run_point_stats`, of the same draws; at least one of the four."""
        arr, nq = _orders_array(orders)
        _lib.check(self.lib.df_flow_point_quantiles(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(n_points),
                                                    C.c_int64(n_draws), C.c_int64(chunk), C.c_uint64(seed),
                                                    C.c_uint64(offset), arr, C.c_int(nq), _ptr(quantbuf),
                                                    _ptr(rankbuf), _ptr(sumsbuf), _ptr(drawsbuf),
                                                    _stream(self.device)), "point_quantiles")

    @staticmethod
    def run_order_statistics(xs, d: int, n_points: int, n_draws: int, orders, out):
        """df_order_statistics on device tensors: see :func:`run_order_statistics`."""
        run_order_statistics(xs, d, n_points, n_draws, orders, out)

    def run_point_histograms(self, thbuf, n_points: int, n_draws: int, chunk: int, seed: int, offset: int, edges=None,
                             bins=None, keep=None, countsbuf=None, drawsbuf=None):
        """df_flow_point_histograms: the draws of :meth:`run_point_stats` counted at the end of
        every chunk.  ``countsbuf`` (int32, n_points blocks of the tables' sizes) takes the tables
        ``keep`` as :func:`run_draw_histograms` lays them out (``edges``, ``bins`` as there),
        ``drawsbuf`` (d · n_points · n_draws) the draws themselves; at least one of the two."""
        barr, karr, nt = _tables_arrays(bins, keep)
        _lib.check(self.lib.df_flow_point_histograms(self.handle, _ptr(thbuf), C.c_int64(n_points), C.c_int64(n_draws),
                                                     C.c_int64(chunk), C.c_uint64(seed), C.c_uint64(offset),
                                                     _ptr(edges), barr, karr, C.c_int32(nt), _ptr(countsbuf),
                                                     _ptr(drawsbuf), _stream(self.device)), "point_histograms")

    @staticmethod
    def run_draw_histograms(xs, d: int, n_points: int, n_draws: int, edges, bins, keep, counts):
        """df_draw_histograms on device tensors: see :func:`run_draw_histograms`."""
        run_draw_histograms(xs, d, n_points, n_draws, edges, bins, keep, counts)

    def run_sample_region(self, xbuf, thvec, n_want: int, lo, hi, A, b, max_tries: int, round: int, seed: int,
                          offset: int = 0):
        """df_flow_sample_region: the first ``n_want`` samples of the (seed, offset) candidate
        stream inside the region into ``xbuf`` → (tried, accepted).  ``lo`` / ``hi``: d host
        floats, ``A`` (n_half, d) and ``b`` (n_half); ``thvec``: ONE n-vector on the device.
        When the slots are not filled within ``max_tries`` the ArgumentError raised carries
        the counts as ``.tried`` and ``.accepted``."""
        lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(-1)
        hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(-1)
        A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, max(lo.shape[0], 1))
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if hi.shape != lo.shape or A.shape[0] != b.shape[0] or (A.shape[0] and A.shape[1] != lo.shape[0]):
            raise _lib.DimensionMismatch("a region needs lo and hi of d values, A of size (n_half, d) and b of n_half")
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        reg = _lib.df_region(lo.shape[0], A.shape[0], fp(lo), fp(hi), fp(A), fp(b))
        tried, accepted = C.c_int64(0), C.c_int64(0)
        rc = self.lib.df_flow_sample_region(self.handle, _ptr(xbuf), _ptr(thvec), C.c_int64(n_want), C.byref(reg),
                                            C.c_int64(max_tries), C.c_int64(round), C.c_uint64(seed),
                                            C.c_uint64(offset), C.byref(tried), C.byref(accepted),
                                            _stream(self.device))
        try:
            _lib.check(rc, "sample_with_rejection")
        except _lib.ArgumentError as e:
            e.tried, e.accepted = tried.value, accepted.value
            raise
        return tried.value, accepted.value

    def random_normal(self, buf, count: int, seed: int, offset: int = 0):
        """df_random_normal: the draw df_flow_sample uses for the same (seed, offset)."""
        _lib.check(self.lib.df_random_normal(_ptr(buf), C.c_int64(count), C.c_uint64(seed), C.c_uint64(offset),
                                             _stream(self.device)), "random_normal")

    # -- array-level API ---------------------------------------------------
    def _inputs(self, y, theta, name):
        yb, dims, was_np = as_julia_device(y, self.d, self.device, name)
        batch = int(np.prod(dims)) if dims else 1
        thb = None
        if self.n > 0:
            if theta is None:
                raise _lib.DimensionMismatch("a conditional flow needs θ of size (n, dims...)")
            thb, tdims, _ = as_julia_device(theta, self.n, self.device, "θ")
            if tdims != dims:
                raise _lib.DimensionMismatch("x and θ must have the same size -- except for the first dimension")
        return yb, thb, dims, batch, was_np

    @staticmethod
    def _ldj_view(buf, dims):
        if not dims:
            return buf.reshape(())
        torch = _torch()
        rev = buf.reshape(tuple(reversed(dims)))
        return rev.permute(*reversed(range(len(dims))))

    def apply(self, op: str, y, theta=None, flow: bool = False):
        """forward / backward → (out, ldj) with the input's logical shape."""
        torch = _torch()
        yb, thb, dims, batch, was_np = self._inputs(y, theta, "input")
        outb, outv = julia_empty(self.d, dims, self.device)
        ldjb = torch.empty(batch, dtype=torch.float32, device=self.device)
        self.run(op, yb, thb, outb, ldjb, batch, flow)
        ldjv = self._ldj_view(ldjb, dims)
        if was_np:
            return _to_numpy(outv), _to_numpy(ldjv)
        return outv, ldjv

    def apply_inplace(self, z, theta=None, flow: bool = False):
        """forward! — mutates ``z`` (a column-major torch tensor) in place."""
        torch = _torch()
        if not isinstance(z, torch.Tensor) or z.device.type != "cuda":
            raise _lib.ArgumentError("forward! needs a device tensor (it mutates its argument)")
        zb, thb, dims, batch, _ = self._inputs(z, theta, "z")
        if zb.data_ptr() != z.data_ptr() or not z.permute(*reversed(range(z.dim()))).is_contiguous():
            raise _lib.ArgumentError("forward! needs z in Julia (column-major) memory order")
        self.run_inplace(zb, thb, batch, flow)
        return None

    def logpdf(self, x, theta=None):
        torch = _torch()
        xb, thb, dims, batch, was_np = self._inputs(x, theta, "x")
        lpb = torch.empty(batch, dtype=torch.float32, device=self.device)
        self.run_logpdf(xb, thb, lpb, batch)
        v = self._ldj_view(lpb, dims)
        return _to_numpy(v) if was_np else v

    def logpdf_sum(self, x, theta=None, out=None):
        torch = _torch()
        xb, thb, dims, batch, _ = self._inputs(x, theta, "x")
        s = out if out is not None else torch.empty(1, dtype=torch.float64, device=self.device)
        self.run_logpdf_sum(xb, thb, s, batch)
        return s, batch


def _to_numpy(t):
    return t.detach().cpu().numpy()
