"""Timing of mpcqp_kinematics and of BatchedController.step at B = 1024 / 4096 (README,
results).  Two questions:

  kinematics   the launch alone: back-to-back eager launches between HIP events (what a
               caller's loop pays per launch, host enqueue included) and 100 launches in a
               captured graph (the device-side cost), against the bandwidth floor of the
               bytes the kernel moves per robot (BYTES_PER_ROBOT) at 6.3 TB/s achievable
  step         a window of 200 control iterations (10 MPC ticks at the reference's
               iterations_between_mpc = 20), ending in a synchronise: ``step`` on the two
               simulator tensors against ``tick`` + ``leg_torques`` fed precomputed
               kinematics, the two alternated so drift hits them alike

Warm-up before every timed window, the median of the repetitions reported with min and
max.  It needs the GPU and does not go through bench.py.  Prints one JSON object and, with
--out, writes it to that file.

  python tools/bench_kinematics.py --out profiles/kinematics/bench_kinematics.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kin_ref  # noqa: E402
from mpcqp.controller import BatchedController  # noqa: E402

DEV = "cuda:0"
# read: root state 13 f32, dof state 24 f32, geometry record 8 f64; written: five [4][3] f32 and [4][3][3] f32
BYTES_PER_ROBOT = 4 * (13 + 24) + 8 * 8 + 4 * (5 * 12 + 36)
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=int, default=200, help="control iterations per timed step window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kinematics needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), bytes_per_robot=BYTES_PER_ROBOT, batches={})
    for B in args.batches:
        rs, ds = (dev(a[0]) for a in kin_ref.make_states(B, 1, seed=B))
        ctl = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        hand = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
        vb, yr = np.array([0.5, 0.0, 0.0]), 0.1
        f_kin = lambda: ctl.engine.kinematics(ctl.geometry, root_states=rs, dof_states=ds, feet=ctl.feet,
                                              thighs=ctl.thighs, pos_feet=ctl.pos_feet,
                                              foot_pos_base=ctl.foot_pos_base, foot_vel_base=ctl.foot_vel_base,
                                              jac=ctl.jac)
        r = dict(kinematics=stats(per_launch(f_kin, n=3000, warm=300, reps=args.reps)))
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                ctl.engine.kinematics(ctl.geometry, root_states=rs, dof_states=ds, feet=ctl.feet, thighs=ctl.thighs,
                                      pos_feet=ctl.pos_feet, foot_pos_base=ctl.foot_pos_base,
                                      foot_vel_base=ctl.foot_vel_base, jac=ctl.jac, stream=s)
        r["kinematics_in_graph"] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
        floor = BYTES_PER_ROBOT * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["kinematics_in_graph"]["median_us"] / floor

        # precomputed kinematics for the by-hand loop: the arrays a caller with its own kinematics holds
        hand.kinematics(rs, ds)
        torch.cuda.synchronize()
        k = {n: getattr(hand, n).clone() for n in kin_ref.OUTPUTS}

        def window_step():
            for it in range(args.window):
                ctl.step(it, vb, yr, rs, ds)

        def window_hand():
            for it in range(args.window):
                hand.tick(it, vb, yr, k["feet"], root_states=rs)
                hand.leg_torques(it, vb, yr, k["thighs"], k["pos_feet"], k["foot_pos_base"], k["foot_vel_base"],
                                 k["jac"], root_states=rs)

        t = dict(step=[], tick_leg_torques=[])
        for _ in range(args.reps):          # alternated; each call is warm-up 1 + one timed window
            t["step"] += [v / args.window for v in per_launch(window_step, n=1, warm=1, reps=1)]
            t["tick_leg_torques"] += [v / args.window for v in per_launch(window_hand, n=1, warm=1, reps=1)]
        r["step_per_iteration"] = stats(t["step"])
        r["tick_leg_torques_per_iteration"] = stats(t["tick_leg_torques"])
        r["step_minus_by_hand_us"] = r["step_per_iteration"]["median_us"] - r["tick_leg_torques_per_iteration"]["median_us"]
        r["tau_bitwise_equal"] = bool(torch.equal(ctl.tau, hand.tau))   # the two loops computed the same thing
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
