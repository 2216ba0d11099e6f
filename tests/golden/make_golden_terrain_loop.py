"""Records the closed loop with the terrain stage on the CPU oracles (tests/terrain_ref.py
closed_loop_terrain: plant_ref.closed_loop with each scenario's plane and the stage under
MPCQP_TERRAIN_GROUND) in tests/golden/terrain_loop.npz: per scenario of terrain_ref.LOOP_SCENARIOS
the figures of terrain_ref.loop_figures, with the stage and (``none_``) without it.
tests/test_terrain_loop.py compares the file with a fresh run and tests/test_gpu_terrain_loop.py
holds the device's loop to its figures.

  python tests/golden/make_golden_terrain_loop.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.dirname(HERE)]
import numpy as np  # noqa: E402

import terrain_ref as tr  # noqa: E402

if __name__ == "__main__":
    out = dict(names=np.array([s[0] for s in tr.LOOP_SCENARIOS]), tilt_rad=np.array([s[1] for s in tr.LOOP_SCENARIOS]),
               azimuth_deg=np.array([s[2] for s in tr.LOOP_SCENARIOS]), command=np.array([s[3] for s in tr.LOOP_SCENARIOS]),
               start_pose=np.array([s[4] for s in tr.LOOP_SCENARIOS]), ticks=np.array(tr.LOOP_TICKS),
               planes=tr.loop_planes(), heights=tr.loop_heights())
    for prefix, stage in (("", True), ("none_", False)):
        run = tr.closed_loop_terrain(stage=stage)
        assert run["solve_ok"].all() and run["finite"].all()
        fig = tr.loop_figures(run)
        for k, v in fig.items():
            out[prefix + k] = v
            print(prefix + k, v)
    np.savez(os.path.join(HERE, "terrain_loop.npz"), **out)
