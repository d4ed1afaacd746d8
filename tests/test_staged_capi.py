"""Staged prediction (tahoe_forest_set_stages, tahoe_forest_predict_staged, tahoe_forest_get_staged_strategy) without a GPU:
the symbols, the NULL-handle refusals, and that the argument checks of set_stages answer before a device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID_ARG = 1
SYMBOLS = ("tahoe_forest_set_stages", "tahoe_forest_predict_staged", "tahoe_forest_get_staged_strategy")


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def test_symbols_are_exported_and_bound(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    for name in SYMBOLS:
        assert name in ta.capi.EXPORTED_SYMBOLS
        assert hasattr(ta.lib, name)
        assert " " + name + "@" in syms or " " + name + "\n" in syms, name  # (the version script tags the names)
        assert name + "(" in header, name
    for method in ("set_stages", "predict_staged", "staged_strategy"):
        assert hasattr(ta.Forest, method) and hasattr(ta.capi.SparseForest, method)
    assert ta.lib.tahoe_abi_version() == 2


def test_null_handle_is_refused(ta):
    rounds = np.array([1, 2, 3], dtype=np.int32)
    assert ta.lib.tahoe_forest_set_stages(None, None, 0) == INVALID_ARG
    assert "null forest" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_set_stages(None, rounds.ctypes.data, 3) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_staged(None, None, None, 0, None) == INVALID_ARG
    assert "null forest" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_predict_staged(None, None, None, 10, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_get_staged_strategy(None, 0) == -1
    assert ta.lib.tahoe_forest_get_staged_strategy(None, 1000) == -1


def test_set_stages_checks_its_arguments_before_a_device_is_touched():
    """In a child process that sees no HIP device: every refusal of set_stages that needs no handle is TAHOE_ERR_INVALID_ARG,
    not TAHOE_ERR_NO_DEVICE or a HIP error, and the process never initialises the runtime for it."""
    code = (
        "import numpy as np, tahoe_amd as ta\n"
        "r = np.array([3, 2, 1], dtype=np.int32)\n"
        "out = [ta.lib.tahoe_forest_set_stages(None, None, 0), ta.lib.tahoe_forest_set_stages(None, None, -1),\n"
        "       ta.lib.tahoe_forest_set_stages(None, None, 3), ta.lib.tahoe_forest_set_stages(None, r.ctypes.data, 3)]\n"
        "print(out, ta.lib.tahoe_last_error().decode())\n"
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    assert res.stdout.startswith("[1, 1, 1, 1] "), res.stdout
    assert "tahoe_forest_set_stages" in res.stdout and "null forest" in res.stdout


def test_python_methods_pass_the_stage_list(ta):
    # the binding turns any sequence of ints into the int32 array of the C call; a NULL handle shows the call was made
    f = ta.Forest.__new__(ta.Forest)
    f._h = C.c_void_p()
    with pytest.raises(ta.TahoeError) as e:
        f.set_stages([1, 2, 5])
    assert e.value.status == INVALID_ARG
    with pytest.raises(ta.TahoeError) as e:
        f.set_stages(None)
    assert e.value.status == INVALID_ARG
    assert f.staged_strategy(100) == -1
