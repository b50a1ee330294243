"""The trainer-chain parameter hand-off, bit for bit ("parameter hand-off").

Every packed weight blob has two writers: the host planner (df_chain_create,
df_chain_set_weights, df_train_create) and the device's repack() after every optimiser update.
tests/test_repack_closure.py closes the nine repack maps on the host; here one parameter vector
p reaches a chain by every route there is, and every route must leave the same bits:

  fresh        load_trainables(chain, p) on a new Python chain, then a new HIPChain
  set_weights  a handle created from the spec's own parameters A, then hc.set_weights
  set_params   a handle from A with a trainer, then tr.set_params(p): the device repack
  stepped      a handle from A with a trainer after 3 steps at B = 64; p := tr.get_params()
  destroyed    the stepped handle after tr.close()

Compared per route, as uint32: forward, forward!, inverse (chain level) and the flow-level
logpdf at B = 289 = 2·128 + 33; the gradient and the fp64 Σ logpdf at B = 300 of the route's
own trainer (a new one for fresh and set_weights); tr.get_params() against p.  The set_weights
and set_params routes also take two vectors of their own: 0.7·U(−1, 1), different from A in
every entry, and that vector with about 1 % of the entries replaced by −0.0, 1e-41, 2**-126,
0.5 + 2**-9 (a bf16 tie), 0.75 and 2**-20, where a device split that flushed subnormals or
rounded ties differently from the host's bf16_split_plane would show.

No tolerance anywhere: the routes are the same arithmetic on what must be the same bytes
(test_deterministic_repeat and the fresh-trainer checks of test_gpu_train_edges.py establish
that the kernels are deterministic).

The last tests hold the library to its contract for a chain that has been trained: a trainer
starts from the parameters its chain evaluates at the moment of creation, whether the trainer
that put them there is gone (the Julia shim's `_trainer!` on a new rule) or alive (two
`setup` calls on one flow).
"""
import re
import time

import numpy as np
import pytest

import densityflows_amd.train as train_mod
import edge_cases as E
import train_edge_cases as T
from densityflows_amd import _lib
from densityflows_amd.train import (Adam, ClipNorm, HIPTrainer, OptimiserChain, load_trainables, setup, train_,
                                    trainables)
from helpers import spec_to_element

pytestmark = pytest.mark.gpu

ENV_KEYS = ("DF_GRID_CUS", "DF_TILES", "DF_SMALL_MAX", "DF_SMALL_WAVES", "DF_F32_EXACT", "DF_NO_WIDE",
            "DF_FORCE_GENERIC", "DF_NO_FAST", "DF_NO_FOLD", "DF_SCORE_PER_NET", "DF_DEBUG_LAUNCH")
LAUNCH = re.compile(r"\[df\] mode (\d+) batch (\d+) kernel (\S+) tiles (\d+) \(max (\d+)\)")
B_PASS = 2 * 128 + 33           # past one workgroup of every chain-pass family
B_GRAD = 300
B_STEP = 64
EDGE_VALUES = np.array([-0.0, 1e-41, 2.0 ** -126, 0.5 + 2.0 ** -9, 0.75, 2.0 ** -20], np.float32)
# the training cases: train_edge_cases.CASES without the config-5 chains but the H0-free one
TRAIN_CASES = [c for c in T.CASES if not c.startswith("cfg5") or c == "cfg5x2_h0free"]


def _flat(a, dev):
    """numpy (rows, B) → flat device buffer in Julia memory order (sample-major)."""
    import torch

    return torch.from_numpy(np.array(np.asarray(a, np.float32).T, order="C").ravel()).to(dev)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32).copy()


class _Case:
    """A structure, its own parameters A (the spec's seed), the environment of its handles and
    its inputs on the device: z / x for the forward / inverse pass and θ (as the chain takes it,
    and raw with the bounds every handle gets) at B_PASS; the gradient's batch; three step
    batches."""

    def __init__(self, spec, d, n, z, x, th, env, sweep, dev, monkeypatch, b_pass=B_PASS):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.spec, self.d, self.n, self.dev, self.b_pass = spec, d, n, dev, b_pass
        self.sweep = getattr(train_mod, "SWEEP_" + sweep)
        self.tmin = (-1.0 - 0.5 * np.arange(n)).astype(np.float32)
        self.tmax = (2.0 + 1.0 * np.arange(n)).astype(np.float32)
        th = np.asarray(th[:, :b_pass], np.float32)
        th_raw = (self.tmin[:, None] + th * (self.tmax - self.tmin)[:, None]).astype(np.float32)
        self.z, self.x = _flat(z[:, :b_pass], dev), _flat(x[:, :b_pass], dev)
        self.th = _flat(th, dev) if n else None
        self.th_raw = _flat(th_raw, dev) if n else None
        gx, gth = T._inputs(d, n, B_GRAD, seed=21)
        self.gx, self.gth = _flat(gx, dev), (_flat(gth, dev) if n else None)
        self.steps = []
        for s in (31, 32, 33):
            sx, sth = T._inputs(d, n, B_STEP, seed=s)
            self.steps.append((_flat(sx, dev), _flat(sth, dev) if n else None))
        self.A = trainables(self.model())
        self.A.setflags(write=False)

    def model(self, p=None):
        chain = spec_to_element(self.spec)
        if p is not None:
            load_trainables(chain, p)
        return chain

    def handle(self, p=None):
        """A new df_chain of the structure holding A, or p."""
        h = self.model(p).hip()
        if self.n:
            h.set_theta_bounds(self.tmin, self.tmax)
        return h

    def trainer(self, h, opt=None):
        tr = HIPTrainer(h, opt or Adam(), sweep=self.sweep)
        tr.set_theta_input(_lib.DF_THETA_GIVEN)
        return tr

    def passes(self, h):
        """forward, forward!, inverse (chain level) and the flow-level logpdf → {name: bits}."""
        import torch

        d, B, dev = self.d, self.b_pass, self.dev
        new = lambda rows: torch.empty(B * rows, dtype=torch.float32, device=dev)
        out = {}
        xb, lb = new(d), new(1)
        h.run("forward", self.z, self.th, xb, lb, B, False)
        out["forward x"], out["forward ldj"] = xb, lb
        zz = self.z.clone()
        h.run_inplace(zz, self.th, B, False)
        out["forward! x"] = zz
        zb, lb2 = new(d), new(1)
        h.run("backward", self.x, self.th, zb, lb2, B, False)
        out["inverse z"], out["inverse ldj"] = zb, lb2
        lp = new(1)
        h.run_logpdf(self.x, self.th_raw, lp, B)
        out["logpdf"] = lp
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in out.items()}

    def grad(self, tr):
        """The gradient and the fp64 Σ logpdf at B_GRAD → {name: bits}."""
        import torch

        lp = torch.zeros(1, dtype=torch.float64, device=self.dev)
        tr.gradient(self.gx, self.gth, B_GRAD, B_GRAD, lp)
        torch.cuda.synchronize()
        return {"gradient": _bits(tr.grad()), "sum logpdf": _bits(lp)}

    def step3(self, tr):
        for sx, sth in self.steps:
            tr.step(sx, sth, B_STEP)

    def vectors(self):
        """The two vectors of the set_weights / set_params routes."""
        rng = np.random.default_rng(77)
        p = (0.7 * (2.0 * rng.random(self.A.shape[0]) - 1.0)).astype(np.float32)
        assert np.all(p != self.A)
        q = p.copy()
        hit = rng.choice(q.shape[0], max(EDGE_VALUES.shape[0], q.shape[0] // 100), replace=False)
        q[hit] = EDGE_VALUES[np.arange(hit.shape[0]) % EDGE_VALUES.shape[0]]
        return {"seeded": p, "edge values": q}


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k} differs in bits")


def _same_params(tr, p, what):
    np.testing.assert_array_equal(tr.get_params().view(np.uint32), np.asarray(p, np.float32).view(np.uint32),
                                  err_msg=f"{what}: get_params() is not the vector, bit for bit")


def _fresh(I, p, opt=None):
    """The reference route: (chain passes, gradient) of a new handle planned from p."""
    h = I.handle(p)
    out = I.passes(h)
    tr = I.trainer(h, opt)
    _same_params(tr, p, "fresh")
    g = I.grad(tr)
    tr.close()
    return out, g


def _stepped(I, opt=None, what=""):
    """The stepped and destroyed routes against fresh; returns the read-back parameters."""
    h = I.handle()
    tr = I.trainer(h, opt)
    _same_params(tr, I.A, f"{what} new trainer")
    I.step3(tr)
    p = tr.get_params()
    assert not np.array_equal(p, I.A) and np.all(np.isfinite(p))
    out, g = I.passes(h), I.grad(tr)
    _same_params(tr, p, f"{what} stepped (after the gradient)")
    ref_out, ref_g = _fresh(I, p, opt)
    _same(out, ref_out, f"{what} stepped against fresh")
    _same(g, ref_g, f"{what} stepped against fresh")
    tr.close()
    _same(I.passes(h), ref_out, f"{what} destroyed against fresh")
    return p, ref_out, ref_g


def _matrix(I, what):
    p, ref_out, ref_g = _stepped(I, what=what)
    routes = {"stepped read-back": (p, ref_out, ref_g)}
    for kind, q in I.vectors().items():
        routes[kind] = (q,) + _fresh(I, q)
    finite = {}
    for kind, (q, ref_out, ref_g) in routes.items():
        finite[kind] = float(np.mean([np.mean(np.isfinite(v.view(np.float32))) for v in ref_out.values()]))
        # set_weights: the host planner writes the blobs of an existing handle
        h = I.handle()
        h.set_weights(I.model(q).layers)
        _same(I.passes(h), ref_out, f"{what} set_weights ({kind}) against fresh")
        tr = I.trainer(h)
        _same_params(tr, q, f"{what} set_weights ({kind})")
        _same(I.grad(tr), ref_g, f"{what} set_weights ({kind}) against fresh")
        tr.close()
        # set_params: the device writes them, the trainer alive
        h = I.handle()
        tr = I.trainer(h)
        tr.set_params(q)
        _same_params(tr, q, f"{what} set_params ({kind})")
        _same(I.passes(h), ref_out, f"{what} set_params ({kind}) against fresh")
        _same(I.grad(tr), ref_g, f"{what} set_params ({kind}) against fresh")
        tr.close()
    return finite


def _chain_case(name, env, dev, monkeypatch, b_pass=B_PASS):
    D = E.case_data(name)
    return _Case(D["spec"], D["d"], D["n"], D["z"], D["x_in"], D["th"], env, "AUTO", dev, monkeypatch, b_pass)


def _train_case(case, dev, monkeypatch):
    chain, sweep, _, env = T.CASES[case]
    spec, d, n, x, th = T.case_data(chain)
    return _Case(spec, d, n, x, x, th, env, sweep, dev, monkeypatch)


@pytest.mark.parametrize("name", list(E.CASES))
def test_chain_pass_routes(cuda, name, monkeypatch):
    """The eleven chain-pass kernel families (tests/edge_cases.py), each under its environment
    and on the kernel it must plan."""
    t0 = time.perf_counter()
    env, kernel_ids = E.CASES[name][3], E.CASES[name][4]
    I = _chain_case(name, env, cuda, monkeypatch)
    kid = I.handle().info.kernel
    assert kid in kernel_ids, f"{name} planned kernel {kid}, expected one of {kernel_ids}"
    finite = _matrix(I, name)
    print(f"HANDOFF chain {name}: kernel {kid} ({E.KERNEL_NAME[kid]}) B {I.b_pass} finite outputs "
          + ", ".join(f"{k} {v:.2f}" for k, v in finite.items()) + f"; {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("small", [True, False])
def test_readme_shape_small_batch_routes(cuda, small, monkeypatch, capfd):
    """The README shape at B = 33: on the small-batch kernel, and with DF_SMALL_MAX=0 on the
    FAST kernel."""
    t0 = time.perf_counter()
    env = dict({} if small else {"DF_SMALL_MAX": "0"}, DF_DEBUG_LAUNCH="1")
    I = _chain_case("fast16", env, cuda, monkeypatch, b_pass=33)
    capfd.readouterr()
    I.passes(I.handle())
    seen = [m.group(3) for m in LAUNCH.finditer(capfd.readouterr().err)]
    assert len(seen) == 4 and set(seen) == {"small" if small else "uniform-fast"}, seen
    _matrix(I, f"fast16 B=33 small={small}")
    capfd.readouterr()
    print(f"HANDOFF chain fast16 B 33 kernel {seen[0]}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_trainer_routes(cuda, case, monkeypatch):
    """One case per training kernel instance (tests/train_edge_cases.py), on the sweep form it
    must run: the trainer's own blobs (transposed fragments, layer-wise blob, the two plane
    blobs) are under the gradient comparison."""
    t0 = time.perf_counter()
    I = _train_case(case, cuda, monkeypatch)
    tr = I.trainer(I.handle())
    form = getattr(train_mod, "SWEEP_" + T.CASES[case][2])
    tr.gradient(I.gx, I.gth, B_GRAD, B_GRAD)        # (the layer-wise form is settled by the first gradient)
    assert tr.sweep() == form, f"{case}: sweep form {tr.sweep()}, expected {T.CASES[case][2]}"
    tr.close()
    finite = _matrix(I, case)
    print(f"HANDOFF train {case}: finite outputs " + ", ".join(f"{k} {v:.2f}" for k, v in finite.items())
          + f"; {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------
# the other ways a step reaches the blobs (README chain; cfg2: the SPLIT blobs)
# ---------------------------------------------------------------------------

CHAINS2 = ["readme", "cfg2"]


def _after(I, h, tr, what):
    """The handle and its live trainer against fresh at the trainer's read-back parameters."""
    p = tr.get_params()
    assert np.all(np.isfinite(p)) and not np.array_equal(p, I.A)
    ref_out, ref_g = _fresh(I, p)
    _same(I.passes(h), ref_out, f"{what} against fresh")
    _same(I.grad(tr), ref_g, f"{what} against fresh")


@pytest.mark.parametrize("case", CHAINS2)
def test_captured_step_then_eager_passes(cuda, case, monkeypatch):
    """df_train_step_graph: eager at first sight, captured, then replayed three times."""
    import torch

    I = _train_case(case, cuda, monkeypatch)
    h = I.handle()
    tr = I.trainer(h)
    xs, ts = I.steps[0][0].clone(), (I.steps[0][1].clone() if I.n else None)
    for k in range(5):
        sx, sth = I.steps[k % 3]
        xs.copy_(sx)
        if I.n:
            ts.copy_(sth)
        tr.step_graph(xs, ts, B_STEP)
    torch.cuda.synchronize()
    _after(I, h, tr, f"{case} captured steps")
    tr.close()


@pytest.mark.parametrize("case", CHAINS2)
def test_epoch_then_eager_passes(cuda, case, monkeypatch):
    """One HIPTrainer.epoch of 4 steps on a resident set."""
    import torch

    I = _train_case(case, cuda, monkeypatch)
    h = I.handle()
    tr = I.trainer(h)
    sx, sth = T._inputs(I.d, I.n, 4 * B_STEP, seed=41)
    assert tr.epoch(_flat(sx, cuda), _flat(sth, cuda) if I.n else None, 4 * B_STEP, None, B_STEP) == 4
    torch.cuda.synchronize()
    _after(I, h, tr, f"{case} epoch")
    tr.close()


@pytest.mark.parametrize("case", CHAINS2)
def test_refused_step_leaves_the_chain_alone(cuda, case, monkeypatch):
    """df_train_set_debug: a step refused for one NaN sample changes neither the parameters nor
    a bit of the chain passes."""
    I = _train_case(case, cuda, monkeypatch)
    h = I.handle()
    tr = I.trainer(h)
    I.step3(tr)
    p, before = tr.get_params(), I.passes(h)
    tr.set_debug(True)
    sx = I.steps[0][0].clone()
    sx[2 + 17 * I.d] = float("nan")
    with pytest.raises(_lib.NonFiniteError):
        tr.step(sx, I.steps[0][1], B_STEP)
    _same_params(tr, p, f"{case} refused step")
    _same(I.passes(h), before, f"{case} after the refused step against before it")
    tr.close()


@pytest.mark.parametrize("case", CHAINS2)
def test_clipnorm_chain_stepped(cuda, case, monkeypatch):
    """OptimiserChain(ClipNorm(1.0), Adam()): the same repack behind another update kernel."""
    I = _train_case(case, cuda, monkeypatch)
    _stepped(I, OptimiserChain(ClipNorm(1.0), Adam()), f"{case} ClipNorm chain")


# ---------------------------------------------------------------------------
# a trainer starts from the parameters its chain evaluates at the moment of creation
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("second", ["same_rule", "other_rule", "first_alive"])
@pytest.mark.parametrize("case", ["readme", "cfg2", "wide_kept"])
def test_second_trainer_starts_from_current_parameters(cuda, case, second, monkeypatch):
    """Trainer 1 steps and goes (first_alive: stays); trainer 2 on the same handle (other_rule:
    Adam(1e-4), the Julia shim's `_trainer!` on a new key) reads back trainer 1's parameters,
    computes the gradient a new trainer on a fresh chain of those parameters computes, and its
    creation changes no bit of the chain passes.  first_alive: two live trainers are allowed;
    each repacks the chain when it steps, so after trainer 2's step the chain evaluates trainer
    2's parameters."""
    t0 = time.perf_counter()
    I = _train_case(case, cuda, monkeypatch)
    rule = Adam(1e-4) if second == "other_rule" else Adam()
    h = I.handle()
    tr1 = I.trainer(h)
    I.step3(tr1)
    p1 = tr1.get_params()
    assert not np.array_equal(p1, I.A)
    before = I.passes(h)
    if second != "first_alive":
        tr1.close()
    tr2 = I.trainer(h, rule)
    _same_params(tr2, p1, f"{case} second trainer ({second})")
    ref_out, ref_g = _fresh(I, p1, rule)
    _same(before, ref_out, f"{case} before the second trainer against fresh")
    _same(I.passes(h), before, f"{case} chain passes after the second trainer's creation against before it")
    _same(I.grad(tr2), ref_g, f"{case} second trainer ({second}) against a new trainer on a fresh chain")
    # ... and it trains on from there: one step of each, bit for bit
    hf = I.handle(p1)
    trf = I.trainer(hf, rule)
    for tr in (tr2, trf):
        tr.step(*I.steps[0], B_STEP)
    p2 = trf.get_params()
    _same_params(tr2, p2, f"{case} second trainer's first step ({second})")
    _same(I.passes(h), I.passes(hf), f"{case} after the second trainer's first step against fresh")
    if second == "first_alive":
        _same_params(tr1, p1, f"{case} the first trainer's own vector")
        tr1.close()     # not the trainer that repacked last: the chain keeps trainer 2's parameters
        _same(I.passes(h), I.passes(hf), f"{case} after the first trainer's destruction")
    tr2.close()
    tr3 = I.trainer(h)
    _same_params(tr3, p2, f"{case} third trainer ({second})")
    tr3.close()
    trf.close()
    print(f"HANDOFF second trainer {case} {second}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("first", ["kept", "closed"])
def test_setup_twice_continues(cuda, first, monkeypatch):
    """The Python API's two-phase use on the datatest fixture (as test_train_runtests_flow):
    setup(Adam(1e-3)) and two epochs, then setup(Adam(1e-4)) on the same flow and one more.
    The second state starts from the model's parameters, and its epoch is bitwise the epoch of
    a fresh flow loaded with the phase-1 parameters."""
    from test_gpu_train import _datatest_flow

    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    t0 = time.perf_counter()
    data, chain, flow = _datatest_flow()
    p0 = trainables(flow.model)
    st1 = setup(Adam(1e-3), flow)
    train_(flow, data, st1, epochs=2, shuffle=False, verbose=False)
    p1 = trainables(flow.model)
    assert not np.array_equal(p1, p0)
    if first == "closed":
        st1.trainer.close()
    st2 = setup(Adam(1e-4), flow)
    _same_params(st2.trainer, p1, "second setup")
    train_(flow, data, st2, epochs=1, shuffle=False, verbose=False)

    data2, chain2, flow2 = _datatest_flow()
    load_trainables(flow2.model, p1)
    flow2.model.invalidate()
    train_(flow2, data2, setup(Adam(1e-4), flow2), epochs=1, shuffle=False, verbose=False)
    assert len(flow.train_loss) == 3 and len(flow2.train_loss) == 1
    print(f"HANDOFF setup twice ({first}): train_loss {flow.train_loss} against {flow2.train_loss}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert flow.train_loss[2] == flow2.train_loss[0] and flow.valid_loss[2] == flow2.valid_loss[0]
    assert flow.train_loss[2] < flow.train_loss[0]          # it continues, it does not start again
    np.testing.assert_array_equal(trainables(flow.model).view(np.uint32), trainables(flow2.model).view(np.uint32))
