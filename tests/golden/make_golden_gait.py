"""Writes tests/golden/gait_switch.npz: the figures of the scheduled closed loop on the
repository's own CPU oracles (tests/gait_ref.closed_loop_scheduled: gait_ref, kin_ref,
oracle.planner, oracle.cpu_port, swing_ref and plant_ref) for the plan gait_ref.PLAN -- Aliengo,
N = 10, iterations_between_mpc = 20, 1400 control iterations, six robots: four that are asked to
change gait at arbitrary ticks, one that trots throughout and one under the automatic choice.
Per robot: the iterations at which it switched, the worst height error, the worst roll / pitch
and the mean forward speed over the last 200 iterations of each phase (padded with nan).
tests/test_gait.py holds the CPU loop to them, tests/test_gpu_gait.py the device loop.

Nothing here comes from the reference: it is this project's oracle output.

    python tests/golden/make_golden_gait.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gait_ref as gr  # noqa: E402


def main():
    run = gr.closed_loop_scheduled(gr.PLAN, gr.PLAN_TICKS)
    assert run["finite"].all() and run["solve_ok"].all()
    err, tilt, speeds = gr.figures(run["x"], run["height"], run["roll"], run["pitch"], run["switch_ticks"], run["dt"])
    B = len(gr.PLAN)
    sw = np.full((B, 2), -1, np.int32)
    sp = np.full((B, 3), np.nan)
    for b in range(B):
        sw[b, :len(run["switch_ticks"][b])] = run["switch_ticks"][b]
        sp[b, :len(speeds[b])] = speeds[b]
    out = os.path.join(HERE, "gait_switch.npz")
    np.savez_compressed(out, switch_ticks=sw, height_error=err, tilt=tilt, phase_speed=sp, ticks=gr.PLAN_TICKS)
    print(out, os.path.getsize(out), "bytes")
    for b in range(B):
        print(f"robot {b}: switches {run['switch_ticks'][b]}, height error {err[b]:.4f} m, roll / pitch {tilt[b]:.4f} rad, "
              f"phase speeds {np.round(speeds[b], 4).tolist()} m/s")


if __name__ == "__main__":
    main()
