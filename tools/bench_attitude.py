"""Timing of mpcqp_attitude and of BatchedEstimator.update_from_imu + BatchedController.step
at B = 1024 / 4096 (README, results).  Two questions:

  attitude     the launch alone: back-to-back eager launches between HIP events (what a
               caller's loop pays per launch, host enqueue included) and 100 launches in a
               captured graph (the device-side cost; also with the trust left out, which
               shows what the four legs' integer phase arithmetic costs), next to the
               bandwidth floor of the bytes the kernel moves per robot (BYTES_PER_ROBOT) at
               6.3 TB/s achievable.
               A robot is one thread and one short dependent chain, so the launch is
               expected to cost what its one-launch neighbours cost (mpcqp_kinematics,
               about 4 us in a graph): the ratio to the floor says how far from bandwidth
  loop         a window of 200 control iterations (10 MPC ticks at the reference's
               iterations_between_mpc = 20), ending in a synchronise: ``est.update_from_imu``
               (attitude + estimate) then ``ctl.step``, against ``est.update`` on a given
               quaternion and trust then ``ctl.step``, the two alternated so drift hits them
               alike

Warm-up before every timed window, the median of the repetitions reported with min and
max.  It needs the GPU and does not go through bench.py.  Prints one JSON object and, with
--out, writes it to that file.

  python tools/bench_attitude.py --out profiles/attitude/bench_attitude.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import att_ref  # noqa: E402
import est_ref  # noqa: E402
import kin_ref  # noqa: E402
from mpcqp.controller import BatchedController  # noqa: E402
from mpcqp.estimator import BatchedEstimator  # noqa: E402

DEV = "cuda:0"
# read and written: the record, 8 f64; read: gyro 3, accel 3, touch 4 f32, tick 1 and gait 9 i32;
# written: quat 4, gyro_out 3, trust 4 f32 and the status word
BYTES_PER_ROBOT = 2 * 8 * 8 + 4 * (3 + 3 + 4) + 4 * (1 + 9) + 4 * (4 + 3 + 4 + 1)
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
        sys.exit("bench_attitude needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), bytes_per_robot=BYTES_PER_ROBOT, batches={})
    for B in args.batches:
        raw = att_ref.make_trajectory(B, 1, seed=B)[0]
        inp = est_ref.make_trajectory(B, 1, seed=B)[0]
        gyro, accel, touch, tick = (dev(raw[k]) for k in ("gyro", "accel", "touch", "tick"))
        quat, trust = dev(inp["quat"]), dev(inp["trust"])
        ds = dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
        ctl = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        told = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        est = BatchedEstimator(B, robot="a1", controller=ctl)
        est_told = BatchedEstimator(B, robot="a1", engine=told.engine)
        eng = ctl.engine

        def f_att(stream=None):
            eng.attitude(est.att_state, gyro, accel, tick=tick, iterations_between_mpc=20, gait=ctl.gait, touch=touch,
                         quat=est.quat, gyro_out=est.gyro_corrected, trust=est.trust, status=est.attitude_status,
                         stream=stream)

        r = dict(attitude=stats(per_launch(f_att, n=2000, warm=200, reps=args.reps)))
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                f_att(stream=s)
        r["attitude_in_graph"] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
        # the orientation tick alone (no gait, no touch, no trust): what the trust's share is
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            for _ in range(100):
                eng.attitude(est.att_state, gyro, accel, quat=est.quat, gyro_out=est.gyro_corrected,
                             status=est.attitude_status, stream=s)
        r["orientation_only_in_graph"] = stats([v / 100 for v in per_launch(g2.replay, n=30, warm=5, reps=args.reps)])
        floor = BYTES_PER_ROBOT * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["attitude_in_graph"]["median_us"] / floor
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else "the latency of the launch and of one robot's chain"
        r["status_ok"] = bool((est.attitude_status == 0).all())

        vb, yr = np.array([0.5, 0.0, 0.0]), 0.1
        est.reset()

        def window_imu():
            for it in range(args.window):
                ctl.step(it, vb, yr, est.update_from_imu(gyro, accel, ds, tick=it), ds)

        def window_told():
            for it in range(args.window):
                told.step(it, vb, yr, est_told.update(quat, gyro, accel, ds, trust), ds)

        t = dict(imu=[], told=[])
        for _ in range(args.reps):          # alternated; each call is warm-up 1 + one timed window
            t["imu"] += [v / args.window for v in per_launch(window_imu, n=1, warm=1, reps=1)]
            t["told"] += [v / args.window for v in per_launch(window_told, n=1, warm=1, reps=1)]
        r["update_from_imu_step_per_iteration"] = stats(t["imu"])
        r["update_step_per_iteration"] = stats(t["told"])
        r["attitude_cost_in_the_loop_us"] = r["update_from_imu_step_per_iteration"]["median_us"] - \
            r["update_step_per_iteration"]["median_us"]
        r["finite"] = bool(torch.isfinite(ctl.tau).all() and torch.isfinite(told.tau).all())
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
