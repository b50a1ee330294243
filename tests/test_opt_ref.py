"""CPU checks of the optimiser chains: the Float32 restatement the GPU tests compare against
(tests/opt_ref.py), the Python rule classes (validation and flattening happen before the
library is touched) and the C ABI's df_opt_rule as the header writes it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
import opt_ref as R
from densityflows_amd import _lib
from densityflows_amd import train as T
from densityflows_amd.train import (Adam, AdamW, ClipGrad, ClipNorm, Descent, OptimiserChain, WeightDecay,
                                    chain_rules)
from oracle import flow_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _vec(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F)


def test_chain_of_adam_is_the_oracle_adam_bitwise():
    n = 517
    offs = np.array([0, 48, 64, 320, 517])
    opt = OptimiserChain(Adam(2e-3, (0.8, 0.99), 1e-7))
    x = _vec(n, 0)
    xo = x.copy()
    st = R.new_state(n, opt)
    sto = [np.zeros(n, F), np.zeros(n, F), (F(0.8), F(0.99))]
    for step in range(3):
        g = _vec(n, 10 + step, 0.3)
        x, _ = R.chain_update(x, g, opt, st, offs)
        O.adam_update(xo, g, sto, eta=F(2e-3), beta=(F(0.8), F(0.99)), eps=F(1e-7))
        assert x.dtype == F and np.array_equal(x, xo)
        assert np.array_equal(st[0], sto[0]) and np.array_equal(st[1], sto[1])
        assert st[2] == sto[2]


def test_clip_grad_by_hand():
    dx = np.array([-2.0, -0.5, -0.25, 0.0, 0.25, 0.5, 3.0, np.nan], F)
    out = R.clip_grad(dx, 0.5)
    assert out.dtype == F
    np.testing.assert_array_equal(out[:7], np.array([-0.5, -0.5, -0.25, 0.0, 0.25, 0.5, 0.5], F))
    assert np.isnan(out[7])                      # Base.clamp passes a NaN through


def test_clip_norm_by_hand():
    offs = np.array([0, 2, 4, 7])
    dx = np.array([3.0, 4.0, 0.3, 0.4, 0.0, 0.0, 0.0], F)      # norms 5, 0.5, 0
    out = R.clip_norm(dx, 1.0, offs)
    np.testing.assert_array_equal(out[:2], dx[:2] * (F(1.0) / F(5.0)))
    assert out[2:4].tobytes() == dx[2:4].tobytes()              # below ω: bit for bit
    assert out[4:].tobytes() == dx[4:].tobytes()                # a zero tensor: nothing divides
    # the bound itself does not clip (nrm > ω is strict)
    assert R.clip_norm(dx, 5.0, offs).tobytes() == dx.tobytes()
    # a NaN norm compares false: dx as it is
    bad = np.array([np.nan, 1.0, 9.0, 0.0, 0.0, 0.0, 0.0], F)
    got = R.clip_norm(bad, 1.0, offs)
    assert np.isnan(got[0]) and got[1] == 1.0 and got[2] == F(9.0) * (F(1.0) / F(9.0))
    # the device's norms take the place of the float64 ones
    np.testing.assert_array_equal(R.clip_norm(dx, 1.0, offs, norms=[F(4.0), F(0.5), F(0.0)])[:2],
                                  dx[:2] * (F(1.0) / F(4.0)))
    np.testing.assert_allclose(R.norms64(dx, offs), [5.0, 0.5, 0.0], rtol=1e-7)


def test_weight_decay_descent_by_hand():
    x = np.array([1.0, -2.0, 0.5], F)
    dx = np.array([0.1, 0.2, -0.3], F)
    np.testing.assert_array_equal(R.weight_decay(dx, x, 0.01), dx + F(0.01) * x)
    np.testing.assert_array_equal(R.descent(dx, 0.5), np.array([0.05, 0.1, -0.15], F))
    xn, d = R.chain_update(x, dx, OptimiserChain(ClipNorm(100.0), Descent(1.0)), R.new_state(3, Descent()),
                           np.array([0, 3]))
    np.testing.assert_array_equal(xn, x - dx)                   # unclipped: x_new = x - g exactly
    # decoupled decay: x -= η·û + λx
    opt = AdamW(1e-3, (0.9, 0.999), 0.1)
    st = R.new_state(3, opt)
    xn, _ = R.chain_update(x, dx, opt, st, np.array([0, 3]))
    st2 = R.new_state(3, Adam())
    upd = R.adam(dx.copy(), st2, 1e-3, (0.9, 0.999), 1e-8)
    np.testing.assert_array_equal(xn, x - (upd + F(0.1) * x))


def test_order_of_rules_matters():
    n = 64
    offs = np.array([0, 64])
    x, g = _vec(n, 1), _vec(n, 2)
    a = OptimiserChain(ClipGrad(0.5), WeightDecay(0.3), Adam())
    b = OptimiserChain(WeightDecay(0.3), ClipGrad(0.5), Adam())
    _, da = R.chain_update(x, g, OptimiserChain(*a.rules[:2], Descent(1.0)), R.new_state(n, Descent()), offs)
    _, db = R.chain_update(x, g, OptimiserChain(*b.rules[:2], Descent(1.0)), R.new_state(n, Descent()), offs)
    assert np.max(np.abs(db)) <= 0.5 < np.max(np.abs(da))
    xa, _ = R.chain_update(x, g, a, R.new_state(n, a), offs)
    xb, _ = R.chain_update(x, g, b, R.new_state(n, b), offs)
    assert not np.array_equal(xa, xb)


def test_pre_clip_dx():
    x, g = _vec(16, 3), _vec(16, 4)
    opt = OptimiserChain(WeightDecay(0.25), ClipNorm(1.0), Adam())
    np.testing.assert_array_equal(R.pre_clip_dx(x, g, opt), g + F(0.25) * x)
    assert R.pre_clip_dx(x, g, OptimiserChain(ClipGrad(1.0), Adam())) is None


# ---- the Python classes -------------------------------------------------------------

def test_chain_flattens_and_exports():
    inner = OptimiserChain(ClipGrad(2.0), OptimiserChain(WeightDecay(1e-3)))
    ch = OptimiserChain(ClipNorm(1.0), inner, Adam())
    assert [type(r) for r in ch.rules] == [ClipNorm, ClipGrad, WeightDecay, Adam]
    kinds = [k for k, _ in chain_rules(ch)]
    assert kinds == [_lib.DF_OPT_CLIP_NORM, _lib.DF_OPT_CLIP_GRAD, _lib.DF_OPT_WEIGHT_DECAY, _lib.DF_OPT_ADAM]
    assert chain_rules(Descent(0.5)) == [(_lib.DF_OPT_DESCENT, (0.5, 0.0, 0.0, 0.0))]
    assert chain_rules(Adam(2e-3, (0.8, 0.99), 1e-7)) == [(_lib.DF_OPT_ADAM, (2e-3, 0.8, 0.99, 1e-7))]
    w = AdamW(1e-3, (0.9, 0.999), 0.01)
    assert isinstance(w, OptimiserChain) and [type(r) for r in w.rules] == [Adam, WeightDecay]
    assert w.rules[1].lam == 0.01 and "OptimiserChain(Adam(" in AdamW.__doc__ and "WeightDecay(" in AdamW.__doc__
    for name in ("ClipGrad", "ClipNorm", "WeightDecay", "Descent", "OptimiserChain", "AdamW", "adjust_"):
        assert getattr(dfa, name) is getattr(T, name)
        assert name in T.__all__


@pytest.mark.parametrize("opt,exc,word", [
    (OptimiserChain(Adam(), Adam()), _lib.UnsupportedError, "Adam"),
    (OptimiserChain(ClipNorm(1.0), ClipNorm(2.0), Adam()), _lib.UnsupportedError, "ClipNorm"),
    (OptimiserChain(Adam(), ClipNorm(2.0)), _lib.UnsupportedError, "ClipNorm"),
    (OptimiserChain(ClipGrad(1.0), WeightDecay(0.1)), _lib.UnsupportedError, "terminal"),
    (OptimiserChain(), _lib.UnsupportedError, "terminal"),
    (OptimiserChain(*([ClipGrad(1.0)] * 8), Adam()), _lib.UnsupportedError, "8 rules"),
    (OptimiserChain(ClipGrad(0.0), Adam()), _lib.ArgumentError, "ClipGrad"),
    (OptimiserChain(ClipGrad(float("nan")), Adam()), _lib.ArgumentError, "ClipGrad"),
    (OptimiserChain(ClipNorm(-1.0), Adam()), _lib.ArgumentError, "ClipNorm"),
    (OptimiserChain(WeightDecay(-1e-3), Adam()), _lib.ArgumentError, "WeightDecay"),
    (OptimiserChain(WeightDecay(float("nan")), Adam()), _lib.ArgumentError, "WeightDecay"),
    (Descent(-0.1), _lib.ArgumentError, "Descent"),
    (OptimiserChain(ClipGrad(1.0), Adam(1e-3, (1.0, 0.999))), _lib.ArgumentError, "Adam"),
    (OptimiserChain(ClipGrad(1.0), "momentum"), _lib.UnsupportedError, "momentum"),
])
def test_structure_errors_are_raised_before_the_library(opt, exc, word):
    with pytest.raises(exc, match=word):
        chain_rules(opt)

    class NoLibrary:                               # a trainer must not reach the library either
        lib = None
        handle = None

    with pytest.raises(exc, match=word):
        T.HIPTrainer(NoLibrary(), opt)


def test_accepted_chains():
    assert len(chain_rules(OptimiserChain(*([ClipGrad(1.0)] * 7), Adam()))) == 8
    assert len(chain_rules(OptimiserChain(Descent(0.1), ClipNorm(1.0), Descent(0.5), Adam()))) == 4
    assert len(chain_rules(OptimiserChain(WeightDecay(0.0), Descent(0.0)))) == 2


# ---- the C ABI as the header writes it ---------------------------------------------------

def _header():
    with open(os.path.join(ROOT, "include", "densityflows_hip.h")) as f:
        return f.read()


def test_opt_rule_layout_matches_the_header():
    h = _header()
    m = re.search(r"typedef struct df_opt_rule \{\s*int32_t kind;\s*float p\[4\];\s*\} df_opt_rule;", h)
    assert m, "df_opt_rule is not {int32_t kind; float p[4];} in the header"
    assert [(n, t) for n, t in _lib.df_opt_rule._fields_] == [("kind", C.c_int32), ("p", C.c_float * 4)]
    assert C.sizeof(_lib.df_opt_rule) == 20 and _lib.df_opt_rule.p.offset == 4
    enum = re.search(r"typedef enum df_opt_kind \{(.*?)\} df_opt_kind;", h, re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(DF_OPT_\w+) = (\d+)", enum)}
    assert vals == {"DF_OPT_ADAM": _lib.DF_OPT_ADAM, "DF_OPT_DESCENT": _lib.DF_OPT_DESCENT,
                    "DF_OPT_CLIP_GRAD": _lib.DF_OPT_CLIP_GRAD, "DF_OPT_CLIP_NORM": _lib.DF_OPT_CLIP_NORM,
                    "DF_OPT_WEIGHT_DECAY": _lib.DF_OPT_WEIGHT_DECAY}
    assert int(re.search(r"#define DF_OPT_MAX_RULES (\d+)", h).group(1)) == _lib.DF_OPT_MAX_RULES == T.MAX_RULES == 8
    r = _lib.df_opt_rule(_lib.DF_OPT_ADAM, (1e-3, 0.9, 0.999, 1e-8))
    assert r.kind == 1 and list(r.p) == [F(1e-3), F(0.9), F(0.999), F(1e-8)]


def test_new_entry_points_are_declared_and_bound():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    want = {"df_train_create_opt": 5, "df_train_adjust": 2, "df_train_num_tensors": 2,
            "df_train_tensor_offsets": 3, "df_train_grad_norms": 3}
    lib = _lib.load()
    for name, nargs in want.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", h)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name)


def test_abi_version_stays_5():
    assert int(re.search(r"#define DF_ABI_VERSION (\d+)", _header()).group(1)) == 5 == _lib.ABI_VERSION
    assert _lib.load().df_get_abi_version() == 5


def test_norm_sum_chain_length_is_the_kernels():
    """GRAD_NORM_K, from which the GPU test derives its tolerance, is the constant the kernel's
    header states and derives (4 accumulators × 64 quads, 2 combining levels, 8 tree levels)."""
    with open(os.path.join(ROOT, "densityflows.jl_amd", "csrc", "df_train.h")) as f:
        m = re.search(r"constexpr int kSumsqK = (\d+) \+ (\d+) \+ (\d+);", f.read())
    assert m and sum(int(v) for v in m.groups()) == T.GRAD_NORM_K == 74
