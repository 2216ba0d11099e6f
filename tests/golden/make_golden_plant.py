"""Writes tests/golden/plant_tau.npz: the joint torques of 200 control iterations of eight
robots, recorded from the repository's own CPU oracle loop (tests/plant_ref.closed_loop: kin_ref,
oracle.planner, oracle.cpu_port, swing_ref and plant_ref) at a forward command of 0.5 m/s on
Aliengo, TROTTING10, N = 10, and the records they start from.  The eight robots start 2 mm apart
in height (0.374 .. 0.388 m), so that their torque sequences and contact events differ.
tests/test_gpu_plant.py replays the torques open loop on the device and on plant_ref.

Nothing here comes from the reference: it is this project's oracle output.

    python tests/golden/make_golden_plant.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import plant_ref as pr  # noqa: E402

TICKS, ROBOTS = 200, 8


def main():
    heights = 0.374 + 0.002 * np.arange(ROBOTS)
    run = pr.closed_loop([0.5] * ROBOTS, TICKS, record_tau=True, heights=heights)
    assert run["finite"].all() and run["solve_ok"].all()
    # the restatement alone keeps all eight clear of every switching threshold
    par = pr.Params()
    st = pr.make_states(ROBOTS, seed=0, par=par)
    rec = run["rec0"].copy()
    for t in range(TICKS):
        near = pr.near_threshold(rec, run["tau"][t], st["robot"], st["geom"], par)
        assert not near.any(), (t, near)
        pr.plant_step(rec, run["tau"][t], st["robot"], st["geom"], par)
    assert np.array_equal(rec, run["rec"])
    out = os.path.join(HERE, "plant_tau.npz")
    np.savez_compressed(out, tau=run["tau"].astype(np.float32), rec0=run["rec0"], rec_end=rec, heights=heights)
    print(out, os.path.getsize(out), "bytes; contact switches per robot:",
          (np.diff(run["touch"], axis=0) != 0).sum((0, 2)))


if __name__ == "__main__":
    main()
