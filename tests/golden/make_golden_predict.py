"""Generate tests/golden/predict.npz FROM THE REFERENCE ITSELF: the state trajectory the
reference's debug branch plots, com_traj = Sx @ xt + Su @ contact_forces
(ModelPredictiveController.__visulize_com_traj_solution, mpc.py:293-294), for the optimum of
the reference-built QP.

Runs only where the reference checkout is (it is read through make_golden.py's stub import; the
tests read the recorded arrays alone).  For N = 10 and 16, six robots each drawn from
mpcqp.synthetic.make_batch (trot, bound, standing; A1 and Aliengo, the records straight from
the reference's config classes), it drives the reference's own

  _generate_state_space_model, _discretize_continuous_model      mpc.py:173-208
  _generate_QP_cost(debug=True)   (keeps Sx, Su, xt)              mpc.py:211-235
  _generate_QP_constraints                                        mpc.py:237-260

and records, per horizon under the key prefix "N{N}_": the inputs (x0, xref, contact, feet,
robot), u* = the exact optimum of that QP (oracle/qp.py dual active set, float64, KKT residuals
asserted, as make_golden.py does), com_traj = c.Sx @ c.xt + c.Su @ u* and the objective
0.5 u*^T H u* + g^T u*.  Arrays only.

Usage:  python tests/golden/make_golden_predict.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "pympc-quadruped_amd")]

from make_golden import stub_reference  # noqa: E402

HORIZONS = (10, 16)
B = 6


def main():
    LinearMpcConfig, robot_configs, mpc, _ = stub_reference(HORIZONS[0])
    from oracle import qp as Q
    from mpcqp.params import robot_from_config
    from mpcqp.synthetic import make_batch
    cfgs = {"a1": robot_configs.A1Config, "aliengo": robot_configs.AliengoConfig}
    out = {}
    for N in HORIZONS:
        LinearMpcConfig.horizon = N          # read by the controller's constructor (mpc.py:39)
        bt = make_batch(B, N, seed=9090 + N, gaits=("trot10", "bound8", "standing"), robots=("a1", "aliengo"))
        us, trajs, objs, names = [], [], [], []
        for b in range(B):
            nm = "a1" if abs(bt["robot"][b][0] - 4.713) < 1e-3 else "aliengo"
            names.append(nm)
            bt["robot"][b] = robot_from_config(cfgs[nm])
            c = mpc.ModelPredictiveController(LinearMpcConfig, cfgs[nm])
            assert c.horizon == N
            c.current_state = bt["x0"][b].copy()
            c.yaw = float(bt["x0"][b][2])
            c.pos_base_feet = [bt["feet"][b][i].astype(np.float64) for i in range(4)]
            Ac, Bc = c._generate_state_space_model()
            Ad, Bd = c._discretize_continuous_model(Ac, Bc)
            H, g = c._generate_QP_cost(Ad, Bd, c.current_state, bt["xref"][b].reshape(-1), debug=True)
            C, lb, ub = c._generate_QP_constraints(bt["contact"][b].reshape(-1))
            u, y, info = Q.solve_qp_dual_active_set(H, g, C, lb, ub)
            k = Q.kkt_residuals(H, g, C, lb, ub, u, y)
            assert max(k["stationarity"], k["primal"], k["dual"], k["complementarity"]) < 1e-7, (N, b, k)
            us.append(u)
            trajs.append(c.Sx @ c.xt + c.Su @ u)                    # mpc.py:294
            objs.append(0.5 * u @ H @ u + g @ u)
        stance = [int(v) for v in (bt["contact"] > 0).reshape(B, -1).sum(1)]
        print(f"N={N}: robots {names}, stance foot-steps {stance}, objective {np.array(objs).round(3)}")
        for key in ("x0", "xref", "contact", "feet", "robot"):
            out[f"N{N}_{key}"] = bt[key]
        out[f"N{N}_u_star"] = np.array(us)
        out[f"N{N}_com_traj"] = np.array(trajs, dtype=np.float64)
        out[f"N{N}_objective"] = np.array(objs, dtype=np.float64)
    out["horizons"] = np.array(HORIZONS)
    out["dt"] = 0.05
    path = os.path.join(HERE, "predict.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
