"""Training — mirror of ``train!`` (src/Flows.jl:380-445) with Optimisers.Adam.

Every step runs on the device through the C ABI (``df_train_*``): the fused
inverse pass keeps each layer's output, the reverse sweep recomputes the
s/t conditioners and back-propagates through the coupling pullbacks
(``rrule(RNVP_backward)`` src/affine/RNVP.jl:99-147, ``rrule(NICE_backward)``
src/affine/NICE.jl:84-113) and the Dense chains on MFMA, gradients are
reduced in a fixed order, then Adam updates the flat parameters and the
packed weights are regathered, so the Flow's forward / logpdf / sample see
the new parameters immediately.  Instead of a bare ``Adam`` the optimiser may be an
``OptimiserChain`` of ``ClipGrad`` / ``ClipNorm`` / ``WeightDecay`` / ``Adam`` / ``Descent``
(``df_train_create_opt``): the whole chain then runs on the device inside ``apply``.

Data parallelism (one process per GPU): :func:`train_` with a
``torch.distributed`` process group shards every batch over the ranks,
computes per-rank gradients with the mean taken over the global batch, and
all-reduces the flat gradient (RCCL over xGMI with the ``nccl`` backend)
before the identical Adam step on every rank.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .hip import HIPChain, _ptr, _stream, as_julia_device, flatten_elements
from .layers import NormalizationLayer, RNVPCouplingLayer

__all__ = ["Adam", "Descent", "ClipGrad", "ClipNorm", "WeightDecay", "OptimiserChain", "AdamW", "setup", "adjust_",
           "TrainState", "HIPTrainer", "train_", "trainables", "load_trainables", "weighted_nll", "check_weights"]


class Adam:
    """``Optimisers.Adam(η = 1f-3, β = (9f-1, 9.99f-1), ϵ = 1f-8)``."""

    def __init__(self, eta: float = 1e-3, beta=(0.9, 0.999), epsilon: float = 1e-8):
        self.eta = float(eta)
        self.beta = (float(beta[0]), float(beta[1]))
        self.epsilon = float(epsilon)

    def __repr__(self):
        return f"Adam(eta={self.eta}, beta={self.beta}, epsilon={self.epsilon})"


class Descent:
    """``Optimisers.Descent(η = 1f-1)``: ``dx = η·dx``."""

    def __init__(self, eta: float = 0.1):
        self.eta = float(eta)

    def __repr__(self):
        return f"Descent(eta={self.eta})"


class ClipGrad:
    """``Optimisers.ClipGrad(δ = 10)``: ``dx = clamp(dx, -δ, δ)`` elementwise."""

    def __init__(self, delta: float = 10.0):
        self.delta = float(delta)

    def __repr__(self):
        return f"ClipGrad(delta={self.delta})"


class ClipNorm:
    """``Optimisers.ClipNorm(ω = 10)`` with p = 2, per parameter tensor (one Dense weight or
    bias): ``nrm = sqrt(Σ dx²)``; where ``nrm > ω``, ``dx = dx·(ω / nrm)``."""

    def __init__(self, omega: float = 10.0):
        self.omega = float(omega)

    def __repr__(self):
        return f"ClipNorm(omega={self.omega})"


class WeightDecay:
    """``Optimisers.WeightDecay(λ = 5f-4)``: ``dx = dx + λ·x``.  Before ``Adam`` in a chain
    it is L2 regularisation, after it decoupled decay."""

    def __init__(self, lam: float = 5e-4):
        self.lam = float(lam)

    def __repr__(self):
        return f"WeightDecay(lam={self.lam})"


class OptimiserChain:
    """``Optimisers.OptimiserChain(rules...)``: every rule in order maps ``dx ← rule(x, dx)``
    from ``dx = ∇``, then ``x ← x - dx``.  Nested chains are flattened.  The device runs
    chains of at most 8 rules with at most one ``Adam``, at most one ``ClipNorm`` (before
    the ``Adam``) and at least one of ``Adam`` / ``Descent``."""

    def __init__(self, *rules):
        self.rules = []
        for r in rules:
            self.rules += r.rules if isinstance(r, OptimiserChain) else [r]

    def __repr__(self):
        return "OptimiserChain(" + ", ".join(repr(r) for r in self.rules) + ")"


def AdamW(eta: float = 1e-3, beta=(0.9, 0.999), lam: float = 0.0, epsilon: float = 1e-8) -> OptimiserChain:
    """``Optimisers.AdamW(η, β, λ, ϵ)``: sugar for
    ``OptimiserChain(Adam(η, β, ϵ), WeightDecay(λ))`` — decoupled decay, ``x -= η·û + λ·x``."""
    return OptimiserChain(Adam(eta, beta, epsilon), WeightDecay(lam))


MAX_RULES = _lib.DF_OPT_MAX_RULES
# the longest chain of Float32 additions behind one tensor's Σ dx² (kSumsqK, csrc/df_train.h):
# grad_norms() is within (GRAD_NORM_K + 3)·2⁻²⁴ of the exact norm, relatively
GRAD_NORM_K = 74


def chain_rules(opt) -> list:
    """The rules of ``opt`` (a rule or an OptimiserChain) as ``(df_opt_kind, (p0..p3))``,
    checked against the device's limits before the library is touched: bad values raise
    ``ArgumentError`` (DF_ERR_INVALID), a structure outside the limits ``UnsupportedError``
    (DF_ERR_UNSUPPORTED).  The message names the rule."""
    rules = opt.rules if isinstance(opt, OptimiserChain) else [opt]
    out = []
    bad = lambda *v: any(not (x >= 0.0) for x in v)  # negative or NaN
    for r in rules:
        if isinstance(r, Adam):
            if bad(r.eta, r.epsilon, *r.beta) or r.beta[0] >= 1.0 or r.beta[1] >= 1.0:
                raise _lib.ArgumentError(f"invalid Adam hyper-parameters: {r!r}")
            out.append((_lib.DF_OPT_ADAM, (r.eta, r.beta[0], r.beta[1], r.epsilon)))
        elif isinstance(r, Descent):
            if bad(r.eta):
                raise _lib.ArgumentError(f"invalid Descent learning rate (η >= 0): {r!r}")
            out.append((_lib.DF_OPT_DESCENT, (r.eta, 0.0, 0.0, 0.0)))
        elif isinstance(r, ClipGrad):
            if not r.delta > 0.0:
                raise _lib.ArgumentError(f"invalid ClipGrad bound (δ > 0): {r!r}")
            out.append((_lib.DF_OPT_CLIP_GRAD, (r.delta, 0.0, 0.0, 0.0)))
        elif isinstance(r, ClipNorm):
            if not r.omega > 0.0:
                raise _lib.ArgumentError(f"invalid ClipNorm bound (ω > 0): {r!r}")
            out.append((_lib.DF_OPT_CLIP_NORM, (r.omega, 0.0, 0.0, 0.0)))
        elif isinstance(r, WeightDecay):
            if bad(r.lam):
                raise _lib.ArgumentError(f"invalid WeightDecay factor (λ >= 0): {r!r}")
            out.append((_lib.DF_OPT_WEIGHT_DECAY, (r.lam, 0.0, 0.0, 0.0)))
        else:
            raise _lib.UnsupportedError(f"OptimiserChain: the device has no rule {r!r}")
    kinds = [k for k, _ in out]
    if len(out) > MAX_RULES:
        raise _lib.UnsupportedError(f"OptimiserChain: more than {MAX_RULES} rules")
    if kinds.count(_lib.DF_OPT_ADAM) > 1:
        raise _lib.UnsupportedError("OptimiserChain: more than one Adam")
    if kinds.count(_lib.DF_OPT_CLIP_NORM) > 1:
        raise _lib.UnsupportedError("OptimiserChain: more than one ClipNorm")
    if _lib.DF_OPT_ADAM not in kinds and _lib.DF_OPT_DESCENT not in kinds:
        raise _lib.UnsupportedError("OptimiserChain: no terminal rule (a chain needs an Adam or a Descent)")
    if (_lib.DF_OPT_CLIP_NORM in kinds and _lib.DF_OPT_ADAM in kinds
            and kinds.index(_lib.DF_OPT_CLIP_NORM) > kinds.index(_lib.DF_OPT_ADAM)):
        raise _lib.UnsupportedError("OptimiserChain: ClipNorm after Adam (it stands before it)")
    return out


class _DeviceArray:
    """A raw device float32 vector exposed to torch via __cuda_array_interface__."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


# reverse-sweep forms (df_sweep_form, include/densityflows_hip.h)
SWEEP_AUTO, SWEEP_FUSED, SWEEP_H0FREE, SWEEP_KEPT, SWEEP_RECOMPUTE, SWEEP_LAYERWISE = 0, 1, 2, 3, 4, 5
SWEEP_SEPARATE = 16
# the form a HIPTrainer requests when none is given (tests set it to exercise one path
# through code that builds its own trainers, e.g. train_)
DEFAULT_SWEEP = SWEEP_AUTO
SWEEP_NAMES = {SWEEP_FUSED: "fused", SWEEP_H0FREE: "h0free", SWEEP_KEPT: "kept", SWEEP_RECOMPUTE: "recompute"}


class HIPTrainer:
    """A ``df_train`` handle bound to a compiled chain (one device).  ``opt``: an ``Adam``
    (df_train_create_ex, the plain Adam kernels) or any other rule / ``OptimiserChain``
    (df_train_create_opt; ``apply`` then runs the whole chain on the device).  ``sweep``: a
    df_sweep_form to request (default: the library picks, SWEEP_AUTO)."""

    def __init__(self, chain: HIPChain, opt, sweep: int | None = None):
        self.chain = chain  # keeps the df_chain alive for this handle's lifetime
        self.lib = chain.lib
        self.opt = opt
        h = C.c_void_p()
        sweep = DEFAULT_SWEEP if sweep is None else sweep
        if not isinstance(opt, Adam):  # any other rule or an OptimiserChain: df_train_create_opt
            rules = chain_rules(opt)
            arr = (_lib.df_opt_rule * len(rules))(*[_lib.df_opt_rule(k, p) for k, p in rules])
            _lib.check(self.lib.df_train_create_opt(C.byref(h), chain.handle, arr, len(rules), int(sweep)),
                       "df_train_create_opt")
        elif sweep == SWEEP_AUTO and not hasattr(self.lib, "df_train_create_ex"):  # a pre-ABI-5 build (A/B runs)
            a = _lib.df_adam(opt.eta, opt.beta[0], opt.beta[1], opt.epsilon)
            _lib.check(self.lib.df_train_create(C.byref(h), chain.handle, C.byref(a)), "df_train_create")
        else:
            a = _lib.df_adam(opt.eta, opt.beta[0], opt.beta[1], opt.epsilon)
            _lib.check(self.lib.df_train_create_ex(C.byref(h), chain.handle, C.byref(a), int(sweep)),
                       "df_train_create_ex")
        self.handle = h
        n = C.c_int64()
        _lib.check(self.lib.df_train_num_params(self.handle, C.byref(n)))
        self.num_params = int(n.value)

    def close(self) -> None:
        """df_train_destroy now (the chain then accepts df_chain_set_weights again)."""
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.df_train_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self.handle = None

    def __del__(self):
        self.close()

    @property
    def device(self):
        return self.chain.device

    def logpdf_grad(self, xbuf, thbuf, batch: int, lp=None, gx=None, gth=None):
        """df_train_logpdf_grad on flat device buffers: per-sample logpdf → ``lp`` (batch,),
        ∂logpdf/∂x → ``gx`` (batch·d, Julia order), ∂logpdf/∂θ → ``gth`` (batch·n); each may be
        None.  θ is read as ``set_theta_input`` says; the trainer's state is left as it is."""
        _lib.check(self.lib.df_train_logpdf_grad(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(lp), _ptr(gx), _ptr(gth),
                                                 C.c_int64(batch), _stream(self.device)), "df_train_logpdf_grad")

    def score_moments(self, xbuf, thbuf, batch: int, out, accumulate: bool = False):
        """df_train_score_moments on flat device buffers: the moment block of ``logpdf_grad``'s lp
        and gθ over the batch into ``out`` (float64 device tensor of 3 + n + n²), overwritten or,
        with ``accumulate``, added to."""
        _lib.check(self.lib.df_train_score_moments(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(batch), _ptr(out),
                                                   1 if accumulate else 0, _stream(self.device)),
                   "df_train_score_moments")

    def fisher(self, thvec, n_samples: int, out, chunk: int = 0, seed: int = 0, offset: int = 0):
        """df_train_fisher: the moment block over ``n_samples`` draws at the ONE raw θ ``thvec``
        (device n-vector, None for n = 0) into ``out`` (float64 device tensor of 3 + n + n²)."""
        _lib.check(self.lib.df_train_fisher(self.handle, _ptr(thvec), C.c_int64(n_samples), C.c_int64(chunk),
                                            C.c_uint64(seed), C.c_uint64(offset), _ptr(out), _stream(self.device)),
                   "df_train_fisher")

    def grad(self):
        """The flat gradient as a torch tensor aliasing the device buffer."""
        import torch

        p = C.c_void_p()
        _lib.check(self.lib.df_train_grad_ptr(self.handle, C.byref(p)))
        return torch.as_tensor(_DeviceArray(p.value or 0, self.num_params), device=self.device)

    def gradient(self, xbuf, thbuf, batch: int, n_total: int = None, lpsum=None, w=None, w_total: float = 0.0,
                 wsums=None):
        """df_train_gradient, or with ``w`` (a float32 device tensor of ``batch`` sample weights)
        df_train_gradient_w: the gradient of ``-Σ w·logpdf / W``.  ``w_total``: 0 for ``W = Σ w``
        of this batch, or the global sum a data-parallel shard divides by; ``wsums``: a float64
        device tensor of 2 for ``{Σ w·logpdf, W}``, or None."""
        if w is not None:
            _check_w_total(w_total)
            _lib.check(self.lib.df_train_gradient_w(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(w), C.c_int64(batch),
                                                    C.c_double(w_total), _ptr(wsums), _stream(self.device)),
                       "df_train_gradient_w")
            return
        _lib.check(self.lib.df_train_gradient(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(batch),
                                              C.c_int64(batch if n_total is None else n_total), _ptr(lpsum),
                                              _stream(self.device)),
                   "df_train_gradient")

    def apply(self):
        _lib.check(self.lib.df_train_apply(self.handle, _stream(self.device)), "df_train_apply")

    def step(self, xbuf, thbuf, batch: int, lpsum=None, w=None, wsums=None):
        """df_train_step; with ``w`` df_train_step_w (``wsums``: see :meth:`gradient`)."""
        if w is not None:
            _lib.check(self.lib.df_train_step_w(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(w), C.c_int64(batch),
                                                _ptr(wsums), _stream(self.device)), "df_train_step_w")
            return
        _lib.check(self.lib.df_train_step(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(batch), _ptr(lpsum),
                                          _stream(self.device)), "df_train_step")

    def step_graph(self, xbuf, thbuf, batch: int, n_total: int = None, lpsum=None, w=None, w_total: float = 0.0,
                   wsums=None):
        """gradient + apply replayed as one hipGraph once the same buffers repeat
        (df_train_step_graph); pass persistent staging buffers.  With ``w`` the weighted step
        (df_train_step_graph_w): ``W`` is summed inside the graph, so the weight buffer may be
        rewritten between calls like ``xbuf``."""
        if w is not None:
            _check_w_total(w_total)
            _lib.check(self.lib.df_train_step_graph_w(self.handle, _ptr(xbuf), _ptr(thbuf), _ptr(w), C.c_int64(batch),
                                                      C.c_double(w_total), _ptr(wsums), _stream(self.device)),
                       "df_train_step_graph_w")
            return
        n_total = batch if n_total is None else n_total
        _lib.check(self.lib.df_train_step_graph(self.handle, _ptr(xbuf), _ptr(thbuf), C.c_int64(batch),
                                                C.c_int64(n_total), _ptr(lpsum), _stream(self.device)),
                   "df_train_step_graph")

    def gather(self, x_out, theta_out, x_set, theta_set, n_samples: int, order, first: int, count: int, w=None):
        """df_batch_gather on flat device buffers: samples ``order[first : first + count]`` of the
        resident set (``x_set`` (n_samples·d,), ``theta_set`` (n_samples·n,), Julia order; ``order``
        an int32 device tensor or None for ``first + j``) into the first ``count`` samples of
        ``x_out`` / ``theta_out``.  ``w``: a pair ``(w_out, w_set)`` of float32 device tensors;
        the set's weights are then gathered in the same launch (df_batch_gather_w)."""
        if w is not None:
            w_out, w_set = w
            _lib.check(self.lib.df_batch_gather_w(_ptr(x_out), _ptr(theta_out), _ptr(w_out), _ptr(x_set),
                                                  _ptr(theta_set), _ptr(w_set), C.c_int(self.chain.d),
                                                  C.c_int(self.chain.n), C.c_int64(n_samples), _ptr(order),
                                                  C.c_int64(first), C.c_int64(count), _stream(self.device)),
                       "df_batch_gather_w")
            return
        _lib.check(self.lib.df_batch_gather(_ptr(x_out), _ptr(theta_out), _ptr(x_set), _ptr(theta_set),
                                            C.c_int(self.chain.d), C.c_int(self.chain.n), C.c_int64(n_samples),
                                            _ptr(order), C.c_int64(first), C.c_int64(count), _stream(self.device)),
                   "df_batch_gather")

    def epoch(self, x_set, theta_set, n_samples: int, order, batchsize: int, step_lp=None, w=None,
              step_wsums=None) -> int:
        """df_train_epoch: one epoch of mini-batch steps on a resident set, enqueued without
        waiting for them.  ``order``: an int32 device tensor of ``n_samples`` indices, or None
        for the set's own order; ``step_lp``: a float64 device tensor with one entry per step
        (ceil(n_samples / batchsize)) for every step's Σ logpdf, or None.  Returns the number of
        steps enqueued, also kept in ``steps_done``; when debug mode refuses a step
        (NonFiniteError), ``steps_done`` is that step's index.  ``w``: the set's weights, a
        float32 device tensor of ``n_samples`` (df_train_epoch_w: every step is the weighted
        step on its gathered weights); ``step_wsums`` then takes 2 float64 per step,
        ``{Σ w·logpdf, W}``."""
        done = C.c_int64(0)
        if w is not None:
            rc = self.lib.df_train_epoch_w(self.handle, _ptr(x_set), _ptr(theta_set), _ptr(w), C.c_int64(n_samples),
                                           _ptr(order), C.c_int64(batchsize), _ptr(step_wsums), C.byref(done),
                                           _stream(self.device))
            self.steps_done = int(done.value)
            _lib.check(rc, "df_train_epoch_w")
            return self.steps_done
        rc = self.lib.df_train_epoch(self.handle, _ptr(x_set), _ptr(theta_set), C.c_int64(n_samples), _ptr(order),
                                     C.c_int64(batchsize), _ptr(step_lp), C.byref(done), _stream(self.device))
        self.steps_done = int(done.value)
        _lib.check(rc, "df_train_epoch")
        return self.steps_done

    def adjust(self, eta: float) -> None:
        """``Optimisers.adjust!(state, η)`` (df_train_adjust): a new η for the chain's Adam, or
        without one its first Descent.  The moments and βᵗ are kept; captured steps are
        re-captured."""
        _lib.check(self.lib.df_train_adjust(self.handle, C.c_float(eta)), "df_train_adjust")
        self.eta = float(eta)

    def tensor_offsets(self) -> np.ndarray:
        """The parameter tensors (one Dense weight or bias each) as slices of the flat vectors:
        count + 1 int64 offsets (df_train_tensor_offsets).  ClipNorm's norms are per tensor."""
        n = C.c_int64()
        _lib.check(self.lib.df_train_num_tensors(self.handle, C.byref(n)), "df_train_num_tensors")
        out = np.empty(int(n.value) + 1, dtype=np.int64)
        _lib.check(self.lib.df_train_tensor_offsets(self.handle, out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    C.c_int64(out.shape[0])), "df_train_tensor_offsets")
        return out

    def grad_norms(self):
        """Per-tensor 2-norms of the gradient buffer as it stands (df_train_grad_norms): a
        float32 device tensor, one entry per tensor of ``tensor_offsets()``."""
        import torch

        n = C.c_int64()
        _lib.check(self.lib.df_train_num_tensors(self.handle, C.byref(n)), "df_train_num_tensors")
        out = torch.empty(int(n.value), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.df_train_grad_norms(self.handle, _ptr(out), _stream(self.device)), "df_train_grad_norms")
        return out

    def sweep(self) -> int:
        """The reverse-sweep form this trainer runs (df_train_sweep: SWEEP_* | SWEEP_SEPARATE)."""
        f = C.c_int()
        _lib.check(self.lib.df_train_sweep(self.handle, C.byref(f)), "df_train_sweep")
        return int(f.value)

    def set_debug(self, on: bool = True) -> None:
        """train!(...; debug=true): refuse the Adam update of a non-finite loss
        (df_train_set_debug → NonFiniteError)."""
        _lib.check(self.lib.df_train_set_debug(self.handle, 1 if on else 0))

    def set_theta_input(self, mode: int) -> None:
        """df_train_set_theta_input: _lib.DF_THETA_AUTO (default; normalise θ iff the
        chain has bounds), DF_THETA_RAW (always normalise) or DF_THETA_GIVEN (never)."""
        _lib.check(self.lib.df_train_set_theta_input(self.handle, int(mode)), "df_train_set_theta_input")

    def allreduce_gradient(self, comm) -> None:
        """Sum the flat gradient over the ranks of ``comm`` (df_train_allreduce_gradient)."""
        _lib.check(self.lib.df_train_allreduce_gradient(self.handle, comm.handle, _stream(self.device)),
                   "df_train_allreduce_gradient")

    def step_dist(self, comm, xbuf, thbuf, batch: int, n_total: int, lpsum=None):
        """One data-parallel step on this rank's shard (df_train_step_dist):
        gradient (mean over the global ``n_total``) → RCCL all-reduce → Adam."""
        _lib.check(self.lib.df_train_step_dist(self.handle, comm.handle if comm is not None else None, _ptr(xbuf),
                                               _ptr(thbuf), C.c_int64(batch), C.c_int64(n_total), _ptr(lpsum),
                                               _stream(self.device)), "df_train_step_dist")

    def get_params(self) -> np.ndarray:
        out = np.empty(self.num_params, dtype=np.float32)
        _lib.check(self.lib.df_train_get_params(self.handle, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                C.c_int64(self.num_params)))
        return out

    def set_params(self, flat) -> None:
        flat = np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        _lib.check(self.lib.df_train_set_params(self.handle, flat.ctypes.data_as(C.POINTER(C.c_float)),
                                                C.c_int64(flat.shape[0])))


def _check_w_total(w_total) -> None:
    if not float(w_total) >= 0.0:  # negative or NaN
        raise _lib.ArgumentError(f"w_total must be 0 (the batch's own Σ w) or > 0, got {w_total!r}")


def check_weights(w, count: int, what: str = "weights") -> np.ndarray:
    """Host-side check of a weight array before the library is touched (the C calls do not
    check, that would synchronise): shape ``(count,)``, every entry finite and >= 0, not all
    zero.  Raises ``ArgumentError`` naming the first offending index; returns float32."""
    w = np.asarray(w)
    if w.ndim != 1 or w.shape[0] != int(count):
        raise _lib.ArgumentError(f"{what} must have shape ({int(count)},), one per sample; got {tuple(w.shape)}")
    w = w.astype(np.float32, copy=False)
    bad = np.flatnonzero(~np.isfinite(w))
    if bad.size:
        raise _lib.ArgumentError(f"{what}[{int(bad[0])}] = {w[bad[0]]} is not finite")
    neg = np.flatnonzero(w < 0)
    if neg.size:
        raise _lib.ArgumentError(f"{what}[{int(neg[0])}] = {w[neg[0]]} is negative")
    if count > 0 and not np.any(w > 0):
        raise _lib.ArgumentError(f"{what}: all {int(count)} weights are zero (index 0 onwards), Σ w must be > 0")
    return np.ascontiguousarray(w)


def weighted_nll(flow, x, theta, w):
    """``(loss, W)`` with ``loss = -Σ w·logpdf / W`` and ``W = Σ w`` over a set, both sums in
    fp64 on the device (df_flow_logpdf_wsum).  ``x`` (d, B), ``theta`` (n, B) or None, ``w``
    (B,): host arrays or device tensors; host weights are checked first (:func:`check_weights`)."""
    import torch

    h = flow.hip()
    dev = h.device
    B = int(x.shape[1])
    if not torch.is_tensor(w):
        w = torch.from_numpy(check_weights(w, B)).to(dev)
    elif w.dim() != 1 or int(w.shape[0]) != B:
        raise _lib.ArgumentError(f"weights must have shape ({B},), one per sample; got {tuple(w.shape)}")
    w = w.to(device=dev, dtype=torch.float32).contiguous()
    xt = as_julia_device(x, flow.d, dev, "x")[0]
    tt = as_julia_device(theta, flow.n, dev, "θ")[0] if flow.n > 0 else None
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    h.run_logpdf_wsum(xt, tt, w, out, B)
    s, W = (float(v) for v in out.cpu().numpy())
    return (-s / W if W > 0 else float("nan")), W


def _dense_order(elements):
    """Dense layers in Flux.trainables order (s_net then t_net per coupling layer)."""
    out = []
    for _, l in flatten_elements(elements):
        if isinstance(l, NormalizationLayer):
            continue
        if isinstance(l, RNVPCouplingLayer):
            out += list(l.s_net)
        out += list(l.t_net)
    return out


def trainables(model) -> np.ndarray:
    """``Flux.trainables(model)`` flattened: per Dense vec(weight) then bias."""
    parts = []
    for D in _dense_order(model.layers):
        parts.append(np.asarray(D.W, np.float32).ravel(order="F"))
        if D.b is not None:
            parts.append(np.asarray(D.b, np.float32))
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def load_trainables(model, flat) -> None:
    """Write a flat trainables vector back into the model's Dense layers."""
    flat = np.asarray(flat, np.float32)
    o = 0
    for D in _dense_order(model.layers):
        k = D.W.size
        D.W = flat[o:o + k].reshape(D.W.shape, order="F").copy()
        o += k
        if D.b is not None:
            D.b = flat[o:o + D.b.size].copy()
            o += D.b.size
    if o != flat.shape[0]:
        raise _lib.DimensionMismatch(f"trainables length {flat.shape[0]} does not match the model ({o})")


class TrainState:
    """``Optimisers.setup(opt, flow.model)``: the device-resident optimiser state."""

    def __init__(self, flow, opt, device=None):
        self.flow = flow
        self.opt = opt
        self.trainer = HIPTrainer(flow.hip(device), opt)

    def sync_model(self):
        """Copy the device parameters back into the Python model (Dense.W / .b)."""
        load_trainables(self.flow.model, self.trainer.get_params())


def setup(opt, flow, device=None) -> TrainState:
    """``Optimisers.setup(opt, flow.model)``; ``opt``: a rule or an ``OptimiserChain``."""
    return TrainState(flow, opt, device)


def adjust_(state: TrainState, eta: float) -> None:
    """``Optimisers.adjust!(state, η)``: a new learning rate, the moments kept (HIPTrainer.adjust)."""
    state.trainer.adjust(eta)


def _dist():
    import torch.distributed as dist

    return dist if dist.is_available() and dist.is_initialized() else None


def _loss(flow, x, th, group=None, comm=None, w=None):
    """loss(backward(model, x, θ)...) over a whole set (fused NLL, fp64 sum).
    With a ``DFComm`` the set is sharded over its ranks and reduced inside the
    library (df_flow_nll); under a bare torch.distributed group (the gloo
    rehearsal) the 16-byte partial goes through torch.  ``w`` (host weights, one per
    sample): the weighted mean ``-Σ w·logpdf / Σ w``, each rank's ``{Σ w·logpdf, Σ w}``
    (df_flow_logpdf_wsum) summed over the ranks."""
    import torch

    from .parallel import allreduce_nll, flow_nll, shard_range

    B = x.shape[1]
    dist = _dist()
    if w is not None:
        if comm is not None:
            a, b = shard_range(B, comm.rank, comm.world)
        elif dist is not None:
            a, b = shard_range(B, dist.get_rank(group), dist.get_world_size(group))
        else:
            a, b = 0, B
        h = flow.hip()
        s = torch.zeros(2, dtype=torch.float64, device=h.device)
        if b > a:
            xt = as_julia_device(x[:, a:b], flow.d, h.device, "x")[0]
            tt = as_julia_device(th[:, a:b], flow.n, h.device, "θ")[0] if th is not None else None
            h.run_logpdf_wsum(xt, tt, torch.from_numpy(np.ascontiguousarray(w[a:b], np.float32)).to(h.device), s, b - a)
        if comm is not None:
            comm.allreduce_(s)
        elif dist is not None:
            dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
        sw, W = (float(v) for v in s.cpu().numpy())
        return -sw / W if W > 0 else float("nan")
    if comm is not None:
        a, b = shard_range(B, comm.rank, comm.world)
        return flow_nll(flow, x[:, a:b], th[:, a:b] if th is not None else None, comm)[0]
    if dist is not None:
        r, w = dist.get_rank(group), dist.get_world_size(group)
        a, b = shard_range(B, r, w)
        x, th = x[:, a:b], (th[:, a:b] if th is not None else None)
    h = flow.hip()
    s = torch.zeros(1, dtype=torch.float64, device=h.device)
    if x.shape[1] > 0:
        h.logpdf_sum(x, th, out=s)
    loss, _, _ = allreduce_nll(s, x.shape[1], group)
    return loss


def _nonfinite(v: float) -> bool:
    return not np.isfinite(v)


def train_(flow, data, state: TrainState, epochs: int = 100, batchsize: int = 64, shuffle: bool = True,
           verbose: bool = True, debug: bool = False, rng=None, group=None, graphs: bool = True, comm=None,
           loader: str = "host", return_step_losses: bool = False):
    """``train!(flow, data, opt_state; epochs, batchsize, shuffle, verbose, debug)`` — src/Flows.jl:380-445.

    Per epoch: mini-batches of the training split (Flux.DataLoader: reshuffled
    every epoch when ``shuffle``, last partial batch kept), one gradient + Adam
    step each; then the train and validation losses are pushed to
    ``flow.train_loss`` / ``flow.valid_loss``.  θ is normalised with the
    Flow's MetaData inside the kernels (= normalized_training_data, Data.jl:189).

    ``debug`` (src/Flows.jl:404-409,423-435): a mini-batch whose loss is NaN
    or ±Inf raises ``ArgumentError`` before its update (the library refuses
    the Adam step, DF_ERR_NONFINITE); a non-finite epoch train / valid loss
    prints the reference's message and returns ``backward(model, set...)``
    = (z, ldj); a run that completes returns (None, None).

    Data parallelism: with ``comm`` (a :class:`DFComm`, one rank per GPU)
    every batch is sharded over its ranks and each step is
    ``df_train_step_dist`` (gradient over the global mean → RCCL all-reduce
    inside the library → Adam); the epoch losses use ``df_flow_nll``.  Under
    a torch.distributed group without ``comm`` (the CPU/gloo rehearsal) the
    gradient goes through torch's all-reduce.  Every rank must pass the same
    ``rng`` seed.  On one device each mini-batch is gathered into a
    persistent staging buffer and the step (reverse sweep, reduction, Adam,
    repack) is replayed as one hipGraph (``graphs``; df_train_step_graph),
    which removes the per-launch host overhead that dominates the reference's
    default batchsize of 64.

    ``loader``: ``"host"`` (the default) builds every mini-batch from the host as described
    above.  ``"device"`` (one device, no ``comm`` / process group) keeps the training and
    validation sets on the device, uploads each epoch's permutation in one copy and runs the
    epoch's steps with one ``df_train_epoch`` call; the two epoch losses are read back
    together, once per epoch.  It draws from ``rng`` as the host loader does, so parameters,
    ``flow.train_loss`` and ``flow.valid_loss`` are bitwise the host loader's.
    ``return_step_losses`` (device loader only): the call returns ``(result, losses)``,
    ``result`` being what it returns otherwise and ``losses`` a float64 numpy array with the
    loss ``-Σ logpdf / B`` of every mini-batch at the parameters before its step.

    Sample weights: with ``DataArrays(..., weights=w)`` every step minimises the mini-batch's
    ``-Σ w·logpdf / Σ w`` on the device (df_train_step_w and its captured / epoch forms) and
    ``flow.train_loss`` / ``flow.valid_loss`` (and the step losses) are the weighted means.
    Data-parallel ranks divide by the global mini-batch's ``Σ w``, taken in fp64 from the
    host's copy, all-reduce the gradient and apply.  Data without weights takes the
    unweighted calls."""
    if loader not in ("host", "device"):
        raise _lib.ArgumentError(f'loader must be "host" or "device", got {loader!r}')
    if loader == "device":
        if comm is not None or _dist() is not None:
            raise _lib.UnsupportedError('loader="device" runs on one device: data-parallel epochs need the '
                                        'gradient all-reduce between the two halves of every step')
        return _train_device(flow, data, state, epochs, batchsize, shuffle, verbose, debug, rng, return_step_losses)
    if return_step_losses:
        raise _lib.UnsupportedError('return_step_losses needs loader="device" (the host loader would have to '
                                    'synchronise at every step to read the loss)')
    import torch

    from .parallel import shard_range

    rng = rng if rng is not None else np.random.default_rng()
    tr = state.trainer
    tr.set_debug(debug)
    dev = tr.device
    x_tr, th_tr = data.training_data()
    x_va, th_va = data.validation_data()
    n = flow.n
    xt, _, _ = as_julia_device(x_tr, flow.d, dev, "x")          # (N*d,) Julia order
    tt = as_julia_device(th_tr, n, dev, "θ")[0] if n > 0 else None
    N = x_tr.shape[1]
    Xs = xt.view(N, flow.d)                                      # row j = sample j
    Ts = tt.view(N, n) if tt is not None else None
    # sample weights (DataArrays(weights=)): the weighted loss on every path below; None:
    # the unweighted calls, untouched
    w_tr, w_va = _data_weights(data, N, x_va.shape[1])
    Ws = torch.from_numpy(w_tr).to(dev) if w_tr is not None else None
    dist = _dist()
    if comm is not None:
        rank, world = comm.rank, comm.world
    else:
        rank, world = (dist.get_rank(group), dist.get_world_size(group)) if dist is not None else (0, 1)
    local = comm is None and dist is None
    staging = {}  # batch size → persistent (x, θ) device buffers (stable pointers for the graphs)
    for _ in range(epochs):
        order = rng.permutation(N) if shuffle else np.arange(N)
        for b0 in range(0, N, batchsize):
            idx = order[b0:b0 + batchsize]
            B = idx.shape[0]
            a, b = shard_range(B, rank, world)
            ii = torch.as_tensor(idx[a:b], device=dev)
            try:
                if local and graphs:
                    if B not in staging:
                        staging[B] = (torch.empty((B, flow.d), dtype=Xs.dtype, device=dev),
                                      torch.empty((B, n), dtype=Ts.dtype, device=dev) if Ts is not None else None,
                                      torch.empty(B, dtype=torch.float32, device=dev) if Ws is not None else None)
                    xb, tb, wb = staging[B]
                    torch.index_select(Xs, 0, ii, out=xb)
                    if Ts is not None:
                        torch.index_select(Ts, 0, ii, out=tb)
                    if Ws is not None:
                        torch.index_select(Ws, 0, ii, out=wb)
                    tr.step_graph(xb, tb, B, w=wb)
                    continue
                xb = Xs.index_select(0, ii).contiguous()
                tb = Ts.index_select(0, ii).contiguous() if Ts is not None else None
                wb = Ws.index_select(0, ii).contiguous() if Ws is not None else None
                if local:
                    tr.step(xb, tb, B, w=wb)
                elif Ws is not None:
                    # every rank divides by the global batch's Σ w (from the host's copy, in
                    # fp64), so the shards' gradients add up to the global batch's
                    w_total = float(np.sum(w_tr[idx], dtype=np.float64))
                    sums = torch.zeros(2, dtype=torch.float64, device=dev)
                    tr.gradient(xb, tb, b - a, w=wb, w_total=w_total, wsums=sums)
                    if comm is not None:
                        tr.allreduce_gradient(comm)
                    else:
                        dist.all_reduce(tr.grad(), op=dist.ReduceOp.SUM, group=group)
                    if debug and dist is not None and comm is None:  # the rehearsal's loss check
                        lp = sums[:1].clone()
                        dist.all_reduce(lp, op=dist.ReduceOp.SUM, group=group)
                        if _nonfinite(float(lp.item()) / w_total):
                            raise _lib.NonFiniteError(f"non-finite training loss {-float(lp.item()) / w_total}")
                    tr.apply()
                elif comm is not None:
                    tr.step_dist(comm, xb, tb, b - a, B)
                else:
                    tr.gradient(xb, tb, b - a, B)
                    dist.all_reduce(tr.grad(), op=dist.ReduceOp.SUM, group=group)
                    if debug:  # the rehearsal's loss check: global Σ logpdf through torch
                        lp = torch.zeros(1, dtype=torch.float64, device=dev)
                        if b > a:
                            flow.hip().logpdf_sum(xb.T, tb.T if tb is not None else None, out=lp)
                        dist.all_reduce(lp, op=dist.ReduceOp.SUM, group=group)
                        if _nonfinite(float(lp.item())):
                            raise _lib.NonFiniteError(f"non-finite training loss {-float(lp.item()) / B}")
                    tr.apply()
            except _lib.NonFiniteError as e:
                # the reference throws from inside the gradient closure, after printing
                # "$l, $ln_det_jac, $z" of the batch (src/Flows.jl:404-409); update! has
                # left flow.model at the last good parameters, and so does sync_model here
                state.sync_model()
                if rank == 0:
                    xv = xb[: b - a].T if local and graphs else xb.T
                    tv = (tb[: b - a].T if local and graphs else tb.T) if tb is not None else None
                    z, ldj = flow.backward(xv, tv)
                    s = flow.hip().logpdf_sum(xv, tv)[0]
                    print(f"{-float(s.item()) / max(b - a, 1)}, {ldj.cpu().numpy()}, {z.cpu().numpy()}")
                raise _lib.ArgumentError(str(e)) from e
        train_loss = _loss(flow, x_tr, th_tr if n > 0 else None, group, comm, w_tr)
        flow.train_loss.append(train_loss)
        if debug and _nonfinite(train_loss):
            if rank == 0:
                print(f"Problem with train loss {train_loss}")
            state.sync_model()
            return _backward_set(flow, x_tr, th_tr)
        valid_loss = _loss(flow, x_va, th_va if n > 0 else None, group, comm, w_va)
        flow.valid_loss.append(valid_loss)
        if debug and _nonfinite(valid_loss):
            if rank == 0:
                print(f"Problem with valid loss {valid_loss}")
            state.sync_model()
            return _backward_set(flow, x_va, th_va)
        if verbose and rank == 0:
            print(f"epoch: {len(flow.train_loss)} | train_loss = {train_loss}, valid_loss = {valid_loss}")
    state.sync_model()
    return (None, None) if debug else None


def _data_weights(data, n_train: int, n_valid: int):
    """The training and validation weights of ``data`` as float32 host arrays, checked, or
    ``(None, None)`` for data without weights."""
    if getattr(data, "weights", None) is None:
        return None, None
    w_tr = check_weights(data.training_weights(), n_train, "training weights")
    w_va = check_weights(data.validation_weights(), n_valid, "validation weights")
    return w_tr, w_va


def _train_device(flow, data, state: TrainState, epochs, batchsize, shuffle, verbose, debug, rng, return_step_losses):
    """``train_(..., loader="device")``: both sets resident on the device, one ``df_train_epoch``
    call and one read-back per epoch."""
    import torch

    if int(batchsize) <= 0:
        raise _lib.ArgumentError("batchsize must be >= 1")
    rng = rng if rng is not None else np.random.default_rng()
    tr = state.trainer
    tr.set_debug(debug)
    dev = tr.device
    n = flow.n
    h = flow.hip()
    x_tr, th_tr = data.training_data()
    x_va, th_va = data.validation_data()
    xt = as_julia_device(x_tr, flow.d, dev, "x")[0]             # (N*d,) Julia order, uploaded once
    tt = as_julia_device(th_tr, n, dev, "θ")[0] if n > 0 else None
    xv = as_julia_device(x_va, flow.d, dev, "x")[0]
    tv = as_julia_device(th_va, n, dev, "θ")[0] if n > 0 else None
    N, Nv = x_tr.shape[1], x_va.shape[1]
    steps = -(-N // int(batchsize))
    order_dev = torch.empty(N, dtype=torch.int32, device=dev) if shuffle else None
    w_tr, w_va = _data_weights(data, N, Nv)
    if w_tr is not None:
        return _train_device_w(flow, state, epochs, int(batchsize), shuffle, verbose, debug, rng, return_step_losses,
                               (x_tr, th_tr, x_va, th_va), (xt, tt, xv, tv), torch.from_numpy(w_tr).to(dev),
                               torch.from_numpy(w_va).to(dev), order_dev)
    # [Σ logpdf of every step | Σ over the training set | Σ over the validation set]: one copy per epoch
    sums = torch.zeros(steps + 2, dtype=torch.float64, device=dev)
    step_losses = []
    ret = lambda r: (r, np.concatenate(step_losses) if step_losses else np.zeros(0)) if return_step_losses else r
    for _ in range(epochs):
        order = rng.permutation(N) if shuffle else None
        if shuffle:
            order_dev.copy_(torch.from_numpy(order.astype(np.int32)))
        try:
            tr.epoch(xt, tt, N, order_dev, batchsize, sums[:steps] if steps else None)
        except _lib.NonFiniteError as e:
            # as the host loader: the model at the last good parameters, the refused batch's
            # diagnostics (rebuilt on the host from the order and the step's index), ArgumentError
            state.sync_model()
            b0 = tr.steps_done * int(batchsize)
            idx = order[b0:b0 + batchsize] if shuffle else np.arange(b0, min(b0 + batchsize, N))
            ii = torch.as_tensor(idx, device=dev)
            xb = xt.view(N, flow.d).index_select(0, ii)
            tb = tt.view(N, n).index_select(0, ii) if tt is not None else None
            xv_, tv_ = xb.T, (tb.T if tb is not None else None)
            z, ldj = flow.backward(xv_, tv_)
            s = flow.hip().logpdf_sum(xv_, tv_)[0]
            print(f"{-float(s.item()) / max(idx.shape[0], 1)}, {ldj.cpu().numpy()}, {z.cpu().numpy()}")
            raise _lib.ArgumentError(str(e)) from e
        sums[steps:].zero_()
        if N > 0:
            h.run_logpdf_sum(xt, tt, sums[steps:steps + 1], N)
        if Nv > 0:
            h.run_logpdf_sum(xv, tv, sums[steps + 1:], Nv)
        got = sums.cpu().numpy()
        if return_step_losses:
            sizes = np.minimum(int(batchsize), N - np.arange(steps) * int(batchsize))
            step_losses.append(-got[:steps] / sizes)
        train_loss = -float(got[steps]) / float(N) if N > 0 else float("nan")
        valid_loss = -float(got[steps + 1]) / float(Nv) if Nv > 0 else float("nan")
        flow.train_loss.append(train_loss)
        if debug and _nonfinite(train_loss):
            print(f"Problem with train loss {train_loss}")
            state.sync_model()
            return ret(_backward_set(flow, x_tr, th_tr))
        flow.valid_loss.append(valid_loss)
        if debug and _nonfinite(valid_loss):
            print(f"Problem with valid loss {valid_loss}")
            state.sync_model()
            return ret(_backward_set(flow, x_va, th_va))
        if verbose:
            print(f"epoch: {len(flow.train_loss)} | train_loss = {train_loss}, valid_loss = {valid_loss}")
    state.sync_model()
    return ret((None, None) if debug else None)


def _train_device_w(flow, state, epochs, batchsize, shuffle, verbose, debug, rng, return_step_losses, host, dev_sets,
                    wt, wv, order_dev):
    """The device loader on a weighted set: the weights resident beside x and θ, gathered per
    step (``df_train_epoch_w``); every sum below comes as the pair ``{Σ w·logpdf, Σ w}``."""
    import torch

    x_tr, th_tr, x_va, th_va = host
    xt, tt, xv, tv = dev_sets
    tr = state.trainer
    dev = tr.device
    n = flow.n
    h = flow.hip()
    N, Nv = x_tr.shape[1], x_va.shape[1]
    steps = -(-N // batchsize)
    # [{Σ w·lp, W} of every step | of the training set | of the validation set]: one copy per epoch
    sums = torch.zeros(2 * (steps + 2), dtype=torch.float64, device=dev)
    step_losses = []
    ret = lambda r: (r, np.concatenate(step_losses) if step_losses else np.zeros(0)) if return_step_losses else r
    for _ in range(epochs):
        order = rng.permutation(N) if shuffle else None
        if shuffle:
            order_dev.copy_(torch.from_numpy(order.astype(np.int32)))
        try:
            tr.epoch(xt, tt, N, order_dev, batchsize, w=wt, step_wsums=sums[:2 * steps] if steps else None)
        except _lib.NonFiniteError as e:
            state.sync_model()
            b0 = tr.steps_done * batchsize
            idx = order[b0:b0 + batchsize] if shuffle else np.arange(b0, min(b0 + batchsize, N))
            ii = torch.as_tensor(idx, device=dev)
            xb = xt.view(N, flow.d).index_select(0, ii)
            tb = tt.view(N, n).index_select(0, ii) if tt is not None else None
            xv_, tv_ = xb.T, (tb.T if tb is not None else None)
            z, ldj = flow.backward(xv_, tv_)
            loss, _ = weighted_nll(flow, xv_, tv_, wt.index_select(0, ii))
            print(f"{loss}, {ldj.cpu().numpy()}, {z.cpu().numpy()}")
            raise _lib.ArgumentError(str(e)) from e
        sums[2 * steps:].zero_()
        if N > 0:
            h.run_logpdf_wsum(xt, tt, wt, sums[2 * steps:2 * steps + 2], N)
        if Nv > 0:
            h.run_logpdf_wsum(xv, tv, wv, sums[2 * steps + 2:], Nv)
        got = sums.cpu().numpy().reshape(steps + 2, 2)
        if return_step_losses:
            step_losses.append(-got[:steps, 0] / got[:steps, 1])
        train_loss = -float(got[steps, 0]) / float(got[steps, 1]) if N > 0 else float("nan")
        valid_loss = -float(got[steps + 1, 0]) / float(got[steps + 1, 1]) if Nv > 0 else float("nan")
        flow.train_loss.append(train_loss)
        if debug and _nonfinite(train_loss):
            print(f"Problem with train loss {train_loss}")
            state.sync_model()
            return ret(_backward_set(flow, x_tr, th_tr))
        flow.valid_loss.append(valid_loss)
        if debug and _nonfinite(valid_loss):
            print(f"Problem with valid loss {valid_loss}")
            state.sync_model()
            return ret(_backward_set(flow, x_va, th_va))
        if verbose:
            print(f"epoch: {len(flow.train_loss)} | train_loss = {train_loss}, valid_loss = {valid_loss}")
    state.sync_model()
    return ret((None, None) if debug else None)


def _backward_set(flow, x, th):
    """``backward(flow.model, set...)`` on a normalised data set: (z, ldj)."""
    return flow.backward(x, th if flow.n > 0 else None)
