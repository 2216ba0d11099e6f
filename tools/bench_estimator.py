"""Timing of mpcqp_estimate and of BatchedEstimator.update + BatchedController.step at
B = 1024 / 4096 (README, results).  Two questions:

  estimate     the launch alone: back-to-back eager launches between HIP events (what a
               caller's loop pays per launch, host enqueue included) and 100 launches in a
               captured graph (the device-side cost), next to the bandwidth floor of the
               bytes the kernel moves per robot (BYTES_PER_ROBOT: the record read and
               written, the sensors, the outputs) at 6.3 TB/s achievable.  The 28 scalar
               updates of a robot run one after the other with a barrier each, so the
               launch may well be bound by that latency and not by the bytes: the ratio
               says which
  loop         a window of 200 control iterations (10 MPC ticks at the reference's
               iterations_between_mpc = 20), ending in a synchronise: ``est.update`` then
               ``ctl.step`` on the estimated root state, against ``ctl.step`` alone on a
               given root state, the two alternated so drift hits them alike

Warm-up before every timed window, the median of the repetitions reported with min and
max.  It needs the GPU and does not go through bench.py.  Prints one JSON object and, with
--out, writes it to that file.

  python tools/bench_estimator.py --out profiles/estimator/bench_estimator.json
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
from mpcqp.controller import BatchedController  # noqa: E402
from mpcqp.estimator import BatchedEstimator  # noqa: E402

DEV = "cuda:0"
# read and written: the record, 352 f64; read: quat 4, gyro 3, accel 3, dof state 24, trust 4 f32 and the
# geometry record 8 f64; written: root state 13, feet 12 f32 and the status word
BYTES_PER_ROBOT = 2 * 352 * 8 + 4 * (4 + 3 + 3 + 24 + 4) + 8 * 8 + 4 * (13 + 12 + 1)
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
        sys.exit("bench_estimator needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), bytes_per_robot=BYTES_PER_ROBOT, batches={})
    for B in args.batches:
        inp = est_ref.make_trajectory(B, 1, seed=B)[0]
        quat, gyro, accel, trust = (dev(inp[k]) for k in ("quat", "gyro", "accel", "trust"))
        ds = dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
        ctl = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        alone = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        est = BatchedEstimator(B, robot="a1", engine=ctl.engine)
        eng = ctl.engine

        def f_est(stream=None):
            eng.estimate(est.est_state, quat, gyro, accel, trust, est.geometry, dof_states=ds,
                         root_states=est.root_states, feet_world=est.feet_world, status=est.status, stream=stream)

        r = dict(estimate=stats(per_launch(f_est, n=2000, warm=200, reps=args.reps)))
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                f_est(stream=s)
        r["estimate_in_graph"] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
        floor = BYTES_PER_ROBOT * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["estimate_in_graph"]["median_us"] / floor
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else "the latency of the 28 sequential updates"
        r["status_ok"] = bool((est.status == 0).all())

        vb, yr = np.array([0.5, 0.0, 0.0]), 0.1
        est.reset()
        est.update(quat, gyro, accel, ds, trust)
        torch.cuda.synchronize()
        rs = est.root_states.clone()

        def window_loop():
            for it in range(args.window):
                ctl.step(it, vb, yr, est.update(quat, gyro, accel, ds, trust), ds)

        def window_alone():
            for it in range(args.window):
                alone.step(it, vb, yr, rs, ds)

        t = dict(loop=[], alone=[])
        for _ in range(args.reps):          # alternated; each call is warm-up 1 + one timed window
            t["loop"] += [v / args.window for v in per_launch(window_loop, n=1, warm=1, reps=1)]
            t["alone"] += [v / args.window for v in per_launch(window_alone, n=1, warm=1, reps=1)]
        r["update_step_per_iteration"] = stats(t["loop"])
        r["step_per_iteration"] = stats(t["alone"])
        r["update_cost_in_the_loop_us"] = r["update_step_per_iteration"]["median_us"] - r["step_per_iteration"]["median_us"]
        r["finite"] = bool(torch.isfinite(ctl.tau).all())
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
