"""Sample weights, host side (no GPU): the two fp64 references of tests/weights_ref.py agree,
`DataArrays(weights=)` partitions the weights with the samples, every Python validation
error is an ArgumentError that names the offending index and is raised before the library
is touched, and the new entry points are declared and bound with matching argument counts."""
import os
import re

import numpy as np
import pytest

import train_edge_cases as T
import weights_ref as W
from densityflows_amd import _lib
from densityflows_amd.data import DataArrays
from densityflows_amd.train import HIPTrainer, check_weights, weighted_nll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"df_train_gradient_w": 8, "df_train_step_w": 7, "df_train_step_graph_w": 8, "df_batch_gather_w": 13,
       "df_train_epoch_w": 10, "df_flow_logpdf_wsum": 7, "df_chain_logpdf_wsum": 7}


def test_the_two_references_agree():
    spec, d, n, x, th = T.case_data("readme")
    B = 12
    k = np.random.default_rng(11).choice([0, 1, 2], size=B, p=[.25, .5, .25])
    assert k.sum() > 0 and (k == 0).any() and (k == 2).any()
    la, ga = W.integer_weight_grad(spec, x[:, :B], th[:, :B], k)
    lb, gb = W.per_sample_grad(spec, x[:, :B], th[:, :B], k)
    assert abs(la - lb) <= 1e-12 * max(1.0, abs(la))
    scale = np.max(np.abs(ga))
    assert scale > 0 and np.max(np.abs(ga - gb)) <= 1e-12 * scale


def test_unit_weights_are_the_unweighted_reference():
    spec, d, n, x, th = T.case_data("readme")
    la, ga = W.integer_weight_grad(spec, x[:, :7], th[:, :7], np.ones(7, np.int64))
    lb, gb = T.oracle_grad("readme", 7)
    assert la == lb and np.array_equal(ga, gb)


def _data(N=40, **kw):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, N)).astype(np.float32)
    th = rng.random((2, N)).astype(np.float32)
    return x, th, DataArrays(x, th, rng=np.random.default_rng(5), **kw)


def test_data_arrays_partition_the_weights():
    w = np.arange(1, 41, dtype=np.float64)
    x, th, data = _data(weights=w)
    assert data.weights.dtype == np.float32
    xt, tt = data.training_data()                      # still two values
    wt, wv = data.training_weights(), data.validation_weights()
    assert wt.shape == (xt.shape[1],) and wv.shape == (data.validation_data()[0].shape[1],)
    assert np.array_equal(wt, w[data.partition.training].astype(np.float32))
    assert np.array_equal(wv, w[data.partition.validation].astype(np.float32))
    # the weight travels with its sample
    assert np.array_equal(xt, x[:, data.partition.training])
    # the same rng gives the same partition with and without weights
    plain = _data()[2]
    assert np.array_equal(plain.partition.training, data.partition.training)
    assert plain.weights is None and plain.training_weights() is None and plain.validation_weights() is None


@pytest.mark.parametrize("bad, index", [
    (lambda w: w.__setitem__(7, np.nan), 7), (lambda w: w.__setitem__(3, np.inf), 3),
    (lambda w: w.__setitem__(11, -0.5), 11)])
def test_data_arrays_refuse_bad_weights(bad, index, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    w = np.ones(40)
    bad(w)
    with pytest.raises(_lib.ArgumentError, match=rf"\[{index}\]"):
        _data(weights=w)


def test_data_arrays_refuse_a_wrong_shape(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    for w in (np.ones(39), np.ones((40, 1)), np.ones((1, 40))):
        with pytest.raises(_lib.ArgumentError, match="shape"):
            _data(weights=w)


def test_data_arrays_refuse_an_all_zero_split(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    part = _data()[2].partition
    w = np.ones(40)
    w[part.validation] = 0.0
    with pytest.raises(_lib.ArgumentError, match=rf"validation split.*index {int(part.validation[0])}\b"):
        _data(weights=w)
    w = np.ones(40)
    w[part.training] = 0.0
    with pytest.raises(_lib.ArgumentError, match=rf"training split.*index {int(part.training[0])}\b"):
        _data(weights=w)
    with pytest.raises(_lib.ArgumentError, match="zero"):
        _data(weights=np.zeros(40))


def test_check_weights():
    assert check_weights([1, 2, 0], 3).dtype == np.float32
    with pytest.raises(_lib.ArgumentError, match=r"shape \(3,\)"):
        check_weights(np.ones(4), 3)
    with pytest.raises(_lib.ArgumentError, match=r"\[1\].*not finite"):
        check_weights([1.0, np.nan, np.inf], 3)
    with pytest.raises(_lib.ArgumentError, match=r"\[2\].*negative"):
        check_weights([1.0, 0.0, -1e-3], 3)
    with pytest.raises(_lib.ArgumentError, match="index 0"):
        check_weights(np.zeros(3), 3)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the weights were checked")


def test_trainer_refuses_a_bad_w_total(monkeypatch):
    tr = HIPTrainer.__new__(HIPTrainer)
    tr.handle = None                                     # (close() at collection does nothing)
    tr.lib = _Untouchable()
    for bad in (-1.0, float("nan")):
        with pytest.raises(_lib.ArgumentError, match="w_total"):
            tr.gradient(None, None, 4, w=object(), w_total=bad)
        with pytest.raises(_lib.ArgumentError, match="w_total"):
            tr.step_graph(None, None, 4, w=object(), w_total=bad)


def test_weighted_nll_checks_host_weights_first():
    class _Flow:
        d, n = 3, 0

        def hip(self):
            class H:
                device = "cpu"
            return H()

    x = np.zeros((3, 5), np.float32)
    for w, pat in ((np.ones(4), "shape"), ([1, 1, np.nan, 1, 1], r"\[2\]"), ([1, 1, 1, -1, 1], r"\[3\]"),
                   (np.zeros(5), "zero")):
        with pytest.raises(_lib.ArgumentError, match=pat):
            weighted_nll(_Flow(), x, None, w)


def _header():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h"), encoding="utf-8").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("name", list(NEW))
def test_header_and_ctypes_table_agree(name):
    m = re.search(r"^\s*int\s+" + name + r"\s*\(([^)]*)\)\s*;", _header(), flags=re.M)
    assert m, f"{name} is not declared in include/densityflows_hip.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
    assert len(_lib.SIGNATURES[name][1]) == len(args) == NEW[name], (name, args)
    assert args[-1] == "void* stream"


def test_abi_version_is_still_5():
    assert _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", _header())
