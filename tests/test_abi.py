"""CPU: the C-ABI library loads, exports every symbol include/mpcqp.h declares,
and its host-side contract holds without a GPU (no compute calls)."""
import ctypes
import os
import re

import pytest

from helpers import INCLUDE, _declared, _prototypes

HEADER = os.path.join(INCLUDE, "mpcqp.h")
# what each header under include/ declares: a count for mpcqp.h, whose names are the table's;
# the names themselves for a companion, which adds to the ABI and keeps its version
HEADERS = {
    "mpcqp.h": 28,
    "mpcqp_predict_abi.h": {"mpcqp_predict"},
    "mpcqp_plant_abi.h": {"mpcqp_plant", "mpcqp_plant_reset", "mpcqp_set_plant"},
    "mpcqp_certify_abi.h": {"mpcqp_certify"},
    "mpcqp_gait_abi.h": {"mpcqp_set_gaits", "mpcqp_set_gait_schedule", "mpcqp_gait_schedule"},
    "mpcqp_disturb_abi.h": {"mpcqp_sensors", "mpcqp_set_sensors", "mpcqp_push"},
}
ARGUMENTS = {"mpcqp_predict": 13, "mpcqp_certify": 13, "mpcqp_plant": 15, "mpcqp_plant_reset": 8,
             "mpcqp_gait_schedule": 15, "mpcqp_sensors": 15, "mpcqp_set_sensors": 13, "mpcqp_push": 8}
_ROLLOUT_ROW = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 10)
ROWS = {"mpcqp_predict": _ROLLOUT_ROW, "mpcqp_certify": _ROLLOUT_ROW}
# what a header's text says beside its declarations
TEXT = {
    "mpcqp_predict_abi.h": ("mpc.py:293-294",),
    "mpcqp_certify_abi.h": ("first-order bound", "tight at the optimum and loose"),
}
# what the comment above each entry point of a header names: what the call replaces
REPLACES = {"mpcqp_gait_abi.h": ("gait.py:", "scripts/mujoco_aliengo.py:121-155")}


def test_header_and_binding_agree():
    from mpcqp import _lib
    assert sorted(_declared()) == sorted(_lib.EXPORTED_SYMBOLS)


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _is_int32(t):
    return t in (ctypes.c_int32, ctypes.c_int) and ctypes.sizeof(t) == 4


# mpcqp.h: a pointer is passed as a pointer (MpcqpParams* as POINTER(MpcqpParams)), int32_t as a 32-bit int
MAIN_RULE = {"T*": _is_pointer, "int32_t": _is_int32, "int": _is_int32, "double": lambda t: t is ctypes.c_double}
# a companion: the context, the stream and every array as c_void_p, each scalar as its own type
COMPANION_RULE = {kind: (lambda t, want=want: t is want) for kind, want in
                  {"T*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "double": ctypes.c_double,
                   "uint64_t": ctypes.c_uint64}.items()}


@pytest.mark.parametrize("header", list(HEADERS))
def test_binding_table_matches_the_header(header):
    """The header declares the functions of its part of the binding table, no other header declares
    one of them, and every row agrees with its declaration position by position: a pointer is
    passed as a pointer, int32_t as a 32-bit int, double as c_double, uint64_t as c_uint64, and
    the return type likewise.  A miscounted row would hand a kernel garbage pointers.  load()
    applied each row to an exported symbol, and the ABI version is the one a companion keeps."""
    from mpcqp import _lib
    main = header == "mpcqp.h"
    assert list(_lib.ABI) == list(HEADERS)
    assert sum(len(rows) for rows in _lib.ABI.values()) == len(_lib.SIGNATURES) == 39    # no name in two parts
    protos, table = _prototypes(header), _lib.ABI[header]
    assert set(protos) == set(table), (header, set(protos) ^ set(table))
    if main:
        assert len(protos) == HEADERS[header], (header, len(protos))
    else:
        assert set(protos) == HEADERS[header], (header, set(protos) ^ HEADERS[header])
    for other in HEADERS:
        twice = set(protos) & set(_prototypes(other)) if other != header else set()
        assert not twice, (header, other, twice)
    agrees = MAIN_RULE if main else COMPANION_RULE
    lib = _lib.load()
    for name, (ret, kinds) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == len(kinds), (name, len(argtypes), len(kinds))
        for i, (kind, t) in enumerate(zip(kinds, argtypes)):
            assert kind in agrees, (name, i, kind)
            assert agrees[kind](t), (name, i, kind, t)
        if not main:
            assert ret == "int" and restype is ctypes.c_int, (name, ret, restype)
        elif ret == "void":
            assert restype is None, name
        elif ret == "T*":
            assert restype is ctypes.c_char_p, name      # the one pointer returned: mpcqp_last_error's text
        else:
            assert ret in ("int", "int32_t") and _is_int32(restype), (name, ret, restype)
        if name in ARGUMENTS:
            assert len(kinds) == ARGUMENTS[name], (name, len(kinds))
        if name in ROWS:
            assert (restype, argtypes) == ROWS[name], name
        # exported, and the table is what load() applies
        assert _lib.SIGNATURES[name] is table[name], name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert lib.mpcqp_abi_version() == _lib.ABI_VERSION == 6       # additive: the ABI version stays
    src = open(os.path.join(INCLUDE, header)).read()
    assert main or '#include "mpcqp.h"' in src, header
    for text in TEXT.get(header, ()):
        assert text in src, (header, text)
    for name in protos if header in REPLACES else ():
        comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", src, re.S).group(1)
        assert all(text in comment for text in REPLACES[header]), name


def test_library_exports_every_declared_symbol():
    from mpcqp import _lib
    lib = _lib.load()
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == _lib.ABI_VERSION == 6


def test_params_struct_layout():
    from mpcqp import _lib
    assert ctypes.sizeof(_lib.MpcqpParams) == 4 + 4 + 8 + 13 * 8 + 12 * 8


def test_default_params_are_the_reference_config():
    """mpcqp_default_params == LinearMpcConfig (linear_mpc_configs.py:4-24) + dt (mpc.py:38)."""
    from mpcqp import _lib
    p = _lib.default_params(16)
    assert p.horizon == 16 and p.dt == 0.05 and p.max_iter == 0
    assert list(p.q_diag) == [5., 5., 10., 10., 10., 50., 0.01, 0.01, 0.2, 0.2, 0.2, 0.2, 0.]
    assert list(p.r_diag) == [1e-5] * 12


def test_create_rejects_bad_arguments_without_crashing():
    from mpcqp import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    p = _lib.default_params(0)   # horizon 0 is invalid
    assert lib.mpcqp_create(ctypes.byref(p), 0, ctypes.byref(ctx)) == -1
    p = _lib.default_params(10)
    # device -1 never exists: an error code, never an exception or a crash
    assert lib.mpcqp_create(ctypes.byref(p), -1, ctypes.byref(ctx)) != 0
    assert lib.mpcqp_solve(None, 1, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mpcqp_set_stance_hint(None, 3) == -1
    assert lib.mpcqp_set_stance_range(None, 1, 3) == -1
    assert lib.mpcqp_set_order(None, 1) == -1
    assert lib.mpcqp_plan(None, 1, 1, *([None] * 15)) == -1
    assert lib.mpcqp_plan_root_states(None, 1, 1, *([None] * 11)) == -1
    assert lib.mpcqp_stance_torques(None, 1, None, None, 4, None, None, None) == -1
    assert lib.mpcqp_set_planner(None, 0.001, 9.81, 0.1) == -1
    assert lib.mpcqp_set_warm_start(None, None, 0) == -1
    assert lib.mpcqp_destroy(None) == 0


def test_header_constants_match_binding():
    """MPCQP_PLAN_STRIDE / GAIT_STRIDE / plan flags are what the Python side uses."""
    from mpcqp import _lib
    src = open(HEADER).read()
    consts = dict(re.findall(r"#define (MPCQP_\w+) (\d+)", src))
    assert int(consts["MPCQP_PLAN_STRIDE"]) == _lib.PLAN_STRIDE
    assert int(consts["MPCQP_GAIT_STRIDE"]) == _lib.GAIT_STRIDE
    assert int(consts["MPCQP_PLAN_REFERENCE"]) == _lib.PLAN_REFERENCE
    assert int(consts["MPCQP_PLAN_NO_INTEGRATE"]) == _lib.PLAN_NO_INTEGRATE
    assert int(consts["MPCQP_ROBOT_STRIDE"]) == _lib.ROBOT_STRIDE
    assert int(consts["MPCQP_WARM_BYTES"]) == _lib.WARM_BYTES == 4 * _lib.MAX_HORIZON


def test_horizon_limit_is_the_create_limit():
    """MPCQP_MAX_HORIZON (include/mpcqp.h) is exactly what mpcqp_create accepts (the
    horizon check runs before any HIP call), and the Python surfaces raise on a longer
    horizon with the limit in the message (linear_mpc_configs.py:11 is a free value)."""
    from mpcqp import _lib, LinearMpc
    src = open(HEADER).read()
    limit = int(re.search(r"#define MPCQP_MAX_HORIZON (\d+)", src).group(1))
    assert limit == _lib.MAX_HORIZON == 32
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    p = _lib.default_params(limit + 1)
    assert lib.mpcqp_create(ctypes.byref(p), 0, ctypes.byref(ctx)) == -1   # MPCQP_ERR_ARG
    p = _lib.default_params(limit)
    rc = lib.mpcqp_create(ctypes.byref(p), 0, ctypes.byref(ctx))
    assert rc != -1   # accepted (no GPU here: MPCQP_ERR_HIP from the device query)
    if rc == 0:
        lib.mpcqp_destroy(ctx)
    with pytest.raises(ValueError, match="1..32"):
        LinearMpc(horizon=limit + 1, device="cuda:0")


def test_gait_records_are_the_reference_gaits():
    """gait.py:16-22 member names -> [period, offsets, durations]."""
    from mpcqp.params import gait_record
    assert gait_record("TROTTING10").tolist() == [10, 0, 5, 5, 0, 5, 5, 5, 5]
    assert gait_record("PACING16").tolist() == [16, 8, 0, 8, 0, 8, 8, 8, 8]
    assert gait_record("bound8").tolist() == [8, 4, 4, 0, 0, 4, 4, 4, 4]
    with pytest.raises(ValueError):
        gait_record((0, (0, 0, 0, 0), (1, 1, 1, 1)))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback: a missing .so is an error, never a silent substitute."""
    from mpcqp import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "absent.so"))
    with pytest.raises(_lib.MpcqpError):
        _lib.load()


def test_engine_refuses_cpu_device():
    torch = pytest.importorskip("torch")
    from mpcqp import LinearMpc
    with pytest.raises(ValueError):
        LinearMpc(horizon=10, device="cpu")
