"""Timing of mpcqp_terrain and of BatchedController.step + BatchedTerrain.update at B = 1024 /
4096 (README, results).  Two questions:

  terrain      the launch alone: back-to-back eager launches between HIP events (what a
               caller's loop pays per launch, host enqueue included) and 100 launches in a
               captured graph (the device-side cost), next to the bandwidth floor of the bytes
               the kernel moves per robot (BYTES_PER_ROBOT: 48 + 16 bytes in, the 160-byte
               record both ways, and the outputs) at 6.3 TB/s achievable.  A robot is one
               thread and one dependent chain of 18 Jacobi rotations, so the launch is
               expected to be bound by latency, like mpcqp_attitude
  loop         a window of 200 control iterations (iterations_between_mpc = 20), ending in a
               synchronise: ``ctl.step`` then ``ter.update()``, against ``ctl.step`` alone on
               a controller with no ground registered, the two alternated so drift hits them
               alike

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_terrain.py --out profiles/terrain/bench_terrain.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import est_ref  # noqa: E402
import kin_ref  # noqa: E402
import terrain_ref  # noqa: E402
from mpcqp import BatchedTerrain  # noqa: E402
from mpcqp.controller import BatchedController  # noqa: E402

DEV = "cuda:0"
# read: pos_feet 12 and contact 4 f32; read and written: the record, 20 f64; written: words 9..11
# of the robot record, normal 3, plane 4, normal_base 3 f32 and the status word (quat 4 f32 read)
BYTES_PER_ROBOT = 4 * (12 + 4) + 2 * 8 * 20 + 4 * (3 + 3 + 4 + 3 + 1) + 4 * 4
HBM_BYTES_PER_S = 6.3e12


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def stats(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v))


def per_launch(fn, n, warm, reps):
    """Microseconds per call of fn over n back-to-back calls between two events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=200, help="control iterations per timed loop window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_terrain needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), bytes_per_robot=BYTES_PER_ROBOT, batches={})
    for B in args.batches:
        step = terrain_ref.make_trajectory(B, 2, seed=B)[1]
        feet, sw, quat = dev(step["pos_feet"]), dev(step["swing_state"]), dev(step["quat"])
        inp = est_ref.make_trajectory(B, 1, seed=B)[0]
        ds = dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
        zero = np.zeros((B, 3), np.float32)
        rs = dev(kin_ref.root_states(inp["quat"], np.tile(np.float32([0, 0, 0.3]), (B, 1)), zero, zero))
        ctl = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        bare = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        ter = BatchedTerrain(B, controller=ctl)
        eng = ctl.engine

        def f_ter(stream=None):
            eng.terrain(ter.terrain_state, feet, swing_state=sw, quat=quat, robot=ctl.robot, normal=ter.normal,
                        plane=ter.plane, normal_base=ter.normal_base, status=ter.status, stream=stream)

        r = dict(terrain=stats(per_launch(f_ter, n=2000, warm=200, reps=args.reps)))
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                f_ter(stream=s)
        r["terrain_in_graph"] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
        floor = BYTES_PER_ROBOT * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["terrain_in_graph"]["median_us"] / floor
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else "the latency of the launch and of one robot's chain"
        r["status_ok"] = bool((ter.status == 0).all())

        vb, yr = np.array([0.5, 0.0, 0.0]), 0.1
        ter.reset()

        def window_terrain():
            for it in range(args.window):
                ctl.step(it, vb, yr, rs, ds)
                ter.update()

        def window_bare():
            for it in range(args.window):
                bare.step(it, vb, yr, rs, ds)

        t = dict(terrain=[], bare=[])
        for _ in range(args.reps):          # alternated; each call is warm-up 1 + one timed window
            t["terrain"] += [v / args.window for v in per_launch(window_terrain, n=1, warm=1, reps=1)]
            t["bare"] += [v / args.window for v in per_launch(window_bare, n=1, warm=1, reps=1)]
        r["step_update_per_iteration"] = stats(t["terrain"])
        r["step_per_iteration"] = stats(t["bare"])
        r["terrain_cost_in_the_loop_us"] = r["step_update_per_iteration"]["median_us"] - \
            r["step_per_iteration"]["median_us"]
        r["finite"] = bool(torch.isfinite(ctl.tau).all() and torch.isfinite(bare.tau).all())
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
