"""GPU: mpcqp_kinematics at its edges -- poses at 0, +-pi, +-pi/2 and 1e4 rad, a straight leg,
a zero, scaled or negated quaternion, a zero geometry, a large base state -- and a NaN in
each input in turn, which must stay where the algebra puts it: a robot is four adjacent
lanes sharing a per-robot LDS slot, 64 robots to a workgroup, so the dirty robots are 63 and
64 of B = 65 and their clean legs are compared bitwise too.  The checks are
tests/kin_edge_checks.py, which tests/test_kin.py runs on the host build of
csrc/mpcqp_kin_leg.h with the same inputs (kin_ref's edge tables); every launch keeps three
sentinel rows past B and finds them untouched.

Bound.  BOUND = 2.4e-7 against kin_ref, norm-wise per robot (tests/test_gpu_kin.py: the
two-ulp float32 floor); an output whose reference is all zero for a robot (zero geometry) is
exactly 0.  On the host the header is within 2.3e-16 (2.7e-16 with R_base supplied) of kin_ref
in float64 on every row and output; after the float32 store feet 3.8e-08, thighs 5.2e-08,
pos_feet 5.5e-08, foot_pos_base 4.1e-08, foot_vel_base 4.4e-08, jac 4.5e-08.  A NaN in
geom[0] or [1] reaches every output but jac, in geom[2] every output, in geom[3] or [4] every
output but thighs, for all four legs (from kin_ref, not hard-coded).
Measured on the MI355X, all twelve rows: split and root layouts feet 3.77e-08, thighs
3.86e-08, pos_feet 5.45e-08, foot_pos_base 3.77e-08, foot_vel_base 4.44e-08, jac 4.52e-08;
with R_base supplied thighs 5.15e-08, foot_pos_base 4.13e-08, foot_vel_base 3.95e-08 -- the
host's figures to the digit; the NaN patterns equal kin_ref's element by element.
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import kin_edge_checks  # noqa: E402
import kin_ref  # noqa: E402
from kin_ref import OUTPUTS  # noqa: E402
from test_gpu_kin import DEV, SENTINEL, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 3


@pytest.fixture(scope="module")
def run():
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=10, robot="aliengo", device=DEV)

    def launch(geom, inp, layout, rot):
        B = len(geom)
        rec = np.zeros((B, kin_ref.STRIDE))
        rec[:, :5] = geom                                     # by hand: pack_leg_geometry refuses a NaN
        g = _dev(rec, torch.float64)
        full = {k: torch.full((B + PAD, 4, 3, 3) if k == "jac" else (B + PAD, 4, 3), SENTINEL, dtype=torch.float32,
                              device=DEV) for k in OUTPUTS}
        outs = {k: v[:B] for k, v in full.items()}
        if layout == "root":
            eng.kinematics(g, root_states=_dev(kin_ref.root_states(inp["quat"], inp["pos"], inp["vel"], inp["omega"])),
                           dof_states=_dev(kin_ref.dof_states(inp["q"], inp["qdot"])), **outs)
        else:
            assert (rot is not None) == (layout == "rot")
            eng.kinematics(g, rot=None if rot is None else _dev(rot, torch.float32),
                           **{k: _dev(inp[k]) for k in ("q", "qdot", "quat", "pos", "vel", "omega")}, **outs)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in full.items()}
        assert all((v[B:] == SENTINEL).all() for v in out.values())
        return out
    return launch


@pytest.mark.parametrize("layout", ["split", "root", "rot"])
def test_edge_poses(run, layout):
    """a.  B = 12 in one launch, all three layouts."""
    worst = kin_edge_checks.check_edge_poses(run, layout)
    print(f"\nedge poses on the device ({layout}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("layout", ["split", "root"])
def test_a_nan_stays_where_the_algebra_puts_it(run, layout):
    """b.  B = 65, dirty robots 63 and 64, one launch per input (and a clean one beside it)."""
    seen = kin_edge_checks.check_nan_stays_put(run, layout)
    assert len(seen) == len(kin_ref.NAN_CASES) - (layout != "split")
