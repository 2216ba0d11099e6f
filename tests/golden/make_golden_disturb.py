"""Records the sensed closed loop on the CPU oracles (tests/disturb_ref.py closed_loop_sensed) in
tests/golden/disturb_loop.npz: per robot of disturb_ref.LOOP_SCALES / LOOP_PUSHES the figures of
disturb_ref.loop_figures.  tests/test_disturb.py compares the file with a fresh run and
tests/test_gpu_disturb.py holds the device's loop to twice its figures.

  python tests/golden/make_golden_disturb.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.dirname(HERE)]
import numpy as np  # noqa: E402

import disturb_ref as dr  # noqa: E402

if __name__ == "__main__":
    run = dr.closed_loop_sensed()
    fig = dr.loop_figures(run["body"], run["est"], run["ok"])
    np.savez(os.path.join(HERE, "disturb_loop.npz"), scales=np.array(dr.LOOP_SCALES), pushes=np.array(dr.LOOP_PUSHES),
             preset=np.array([dr.MEMS[k] for k in sorted(dr.MEMS)]), **fig)
    for k, v in fig.items():
        print(k, v)
