"""Device-resident epochs, host side (no GPU): the two entry points are declared in the
header and bound in ``_lib`` with matching argument counts, ``train_`` refuses a bad
``loader`` before it touches the library, and the ABI version has not moved."""
import os
import re

import pytest

from densityflows_amd import _lib
from densityflows_amd.train import train_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("df_batch_gather", "df_train_epoch")


def _header():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h"), encoding="utf-8").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared_args(name):
    m = re.search(r"^\s*int\s+" + name + r"\s*\(([^)]*)\)\s*;", _header(), flags=re.M)
    assert m, f"{name} is not declared in include/densityflows_hip.h"
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", NEW)
def test_header_and_ctypes_table_agree(name):
    args = _declared_args(name)
    assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == len(args), (name, len(argtypes), args)
    assert args[-1] == "void* stream"


def test_declared_shapes():
    assert len(_declared_args("df_batch_gather")) == 11
    assert len(_declared_args("df_train_epoch")) == 9
    assert _declared_args("df_train_epoch")[0] == "df_train* t"


def test_the_makefile_builds_the_new_unit():
    mk = open(os.path.join(ROOT, "densityflows.jl_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "df_epoch.hip" in mk
    src = open(os.path.join(ROOT, "densityflows.jl_amd", "csrc", "df_epoch.hip"), encoding="utf-8").read()
    for k in ("batch_gather_kernel", "order_range_kernel", "cursor_advance_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\b", src), k


def test_abi_version_is_still_5():
    assert _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", _header())


class _Untouchable:
    """Stands in for flow, data and state: any use of it is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"train_ touched .{name} before checking its loader argument")


def test_unknown_loader_is_an_argument_error(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    u = _Untouchable()
    for bad in ("Device", "gpu", "", None, 1):
        with pytest.raises(_lib.ArgumentError):
            train_(u, u, u, loader=bad)


def test_device_loader_refuses_data_parallelism(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    u = _Untouchable()
    with pytest.raises(_lib.UnsupportedError):
        train_(u, u, u, loader="device", comm=object())


def test_device_loader_refuses_an_initialised_process_group(monkeypatch):
    import densityflows_amd.train as train_mod

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    monkeypatch.setattr(train_mod, "_dist", lambda: object())
    u = _Untouchable()
    with pytest.raises(_lib.UnsupportedError):
        train_(u, u, u, loader="device")


def test_step_losses_need_the_device_loader(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    u = _Untouchable()
    with pytest.raises(_lib.UnsupportedError):
        train_(u, u, u, return_step_losses=True)
