"""GPU: mpcqp_terrain at its edges -- the checks of tests/terrain_edge_checks.py, which
tests/test_terrain.py runs on the host build of the same text, on the device: held fits
(collinear, coincident, thin, too steep, vertical) from a fresh and from a tilted record, the
blend against the restatement and caller-seeded normals, exact structure (a diagonal scatter, a
double eigenvalue, normals near an axis, scaling by powers of two bitwise), thin but accepted
footprints, the decisions on odd contact values and non-finite feet, the refusals by the record,
feet 1e4 and 1e5 m from the origin, and MPCQP_TERRAIN_GROUND.

B = W + 3 = 67 robots, one case each in turn, so every case also sits in the tail workgroup; the
record, every output and the robot records lie between canary rows that every launch leaves
untouched.  Bounds as tests/test_gpu_terrain.py: N_BOUND = 1.1e-14 for the record, F32_BOUND =
2.4e-7 for a float32 output; a thin footprint of spread s < 0.05 gets N_BOUND 0.05 / s.

Measured on the MI355X: see DESIGN.md 4.4g (the tests print the figures).
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import terrain_edge_checks as edge  # noqa: E402
import terrain_ref as tr  # noqa: E402
import test_gpu_terrain as T  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

_engines = {}


def _engine(constants):
    key = tuple(sorted((constants or {}).items()))
    if key not in _engines:
        _engines[key] = T.engine(**(constants or {}))
    return _engines[key]


def launch(state, inp, constants=None, ground=False):
    """One eng.terrain call on a copy of ``state`` between canary rows; returns the B rows."""
    eng = _engine(constants)
    B = len(state)
    bf = T.buffers(B)
    T.live(bf, "state", B).copy_(_dev(np.asarray(state, np.float64)))
    kw = {}
    if "robot" in inp:
        bf["robot"] = torch.full((T.FRONT + B + 2, 16), T.CANARY, device=DEV)
        T.live(bf, "robot", B).copy_(_dev(np.asarray(inp["robot"], np.float32)))
        kw["robot"] = T.live(bf, "robot", B)
    for k in ("contact", "swing_state", "quat", "root_states"):
        if inp.get(k) is not None:
            kw[k] = _dev(np.asarray(inp[k], np.float32))
    skip = () if ("quat" in kw or "root_states" in kw) else ("normal_base",)
    kw.update({k: T.live(bf, k, B) for k in T.OUTPUTS if k not in skip})
    eng.terrain(T.live(bf, "state", B), _dev(np.asarray(inp["pos_feet"], np.float32)), ground=ground, **kw)
    torch.cuda.synchronize()
    o = T.read(bf)
    for k, v in o.items():
        assert (v[B:] == T.CANARY).all(), (k, "canary")
    assert all((o[k] == T.CANARY).all() for k in skip)
    return o["state"][:B].copy(), {k: v[:B] for k, v in o.items() if k != "state"}


@pytest.fixture(scope="module")
def traj():
    return tr.make_trajectory(**tr.GPU_TRAJECTORY)


def test_held_fits():
    print(f"\nheld fits: d and accepted n against the restatement {edge.check_held_fits(launch):.2e} of the bound")


def test_blend_and_seeded_normals(traj):
    print(f"\nblend 0.25 / 0.5 over 10 ticks: {edge.check_blend(launch, traj):.2e} (bound {edge.N_BOUND:.1e})")
    edge.check_seeded_normals(launch)


def test_exact_structure_and_scaling():
    w = edge.check_exact_structure(launch)
    rows = edge.check_scaling(launch)
    print(f"\nexact structure {w:.2e} of the bound; {rows} scaled rows bitwise")


def test_thin_footprints():
    err = edge.check_thin_footprints(launch)
    print("\nthin footprints, spread: error (bound)  " + "  ".join(
        f"{s}: {e:.2e} ({edge.N_BOUND * max(1, 0.05 / s):.1e})" for s, e in err.items()))


def test_odd_inputs():
    edge.check_odd_inputs(launch)


def test_bad_records():
    print(f"\nrefused records: {edge.check_bad_records(launch)}")


def test_far_from_the_origin():
    worst, fitted = edge.check_far_from_the_origin(launch)
    print(f"\n1e4 / 1e5 m from the origin: {worst:.2e} (bound {edge.N_BOUND:.1e}); share fitted per tick {fitted}")


def test_ground_flag(traj):
    print(f"\nground flag: plane word against d - n_z touchdown_z {edge.check_ground_flag(launch, traj):.2e}")
