"""CPU: mpcqp_step, the control tick in one call, is declared, exported and bound, is an
additive change to the ABI (the version stays 6), and refuses a NULL context without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")


def test_step_is_declared_exported_and_bound():
    from mpcqp import _lib
    assert "mpcqp_step" in _lib.EXPORTED_SYMBOLS
    src = open(HEADER).read()
    decl = re.search(r"^int mpcqp_step\((.*?)\);", src, re.M | re.S)
    assert decl, "include/mpcqp.h declares no mpcqp_step"
    lib = _lib.load()
    assert hasattr(lib, "mpcqp_step")
    # one ctypes argument type per declared parameter
    assert len(lib.mpcqp_step.argtypes) == len(decl.group(1).split(",")) == 33
    assert lib.mpcqp_step.restype is ctypes.c_int


def test_abi_version_is_unchanged():
    from mpcqp import _lib
    assert _lib.load().mpcqp_abi_version() == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define MPCQP_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 6


def test_step_refuses_a_null_context():
    from mpcqp import _lib
    lib = _lib.load()
    for flags in (0, _lib.STEP_MPC):
        assert lib.mpcqp_step(None, 1, flags, 0, None, 20, *([None] * 27)) == _lib.ERR_ARG


def test_step_flag_matches_the_header():
    from mpcqp import _lib
    consts = dict(re.findall(r"#define (MPCQP_\w+) (\d+)", open(HEADER).read()))
    assert int(consts["MPCQP_STEP_MPC"]) == _lib.STEP_MPC == 1


def test_python_surfaces_exist():
    from mpcqp import LinearMpc
    from mpcqp.controller import BatchedController
    assert callable(LinearMpc.step) and callable(LinearMpc.bind_step)
    assert callable(BatchedController.step_fused) and callable(BatchedController.set_command)
