"""Timing of mpcqp_gait_schedule at B = 1024 / 4096 (README, results).  Two
questions:

  schedule     the launch alone, eager (back-to-back launches between HIP events: what a caller's
               loop pays per launch, host enqueue included) and 100 launches in a captured graph
               (the device-side cost), in three states of the fleet:
                 idle       no request pending: every robot advances its clock and stores its tick
                            and the first half of its record
                 waiting    the worst case: every robot has a request pending on an aligned tick
                            that is not a seam (trot10 at tick 40, two legs mid-swing, asked for
                            pace10; launched without MPCQP_GAIT_ADVANCE so that the tick stays
                            there), so every robot pays the tick's remainder, its gait record and
                            swing_counts' 64-bit remainders, and nobody switches
                 iteration  idle, with the `iteration` output, which costs every robot divisions
               and beside each, in the same process, mpcqp_attitude without the trust -- the
               closest existing kernel in shape, one thread per robot and a small record
  iteration    a control iteration of the closed loop: ``step_fused; plant.step`` against
               ``sched.update; step_fused; plant.step`` (the tick then lives on the device),
               windows of 20 iterations (one MPC tick and 19 ticks between two solves) ending in a
               synchronise, the two alternated so drift hits them alike (DESIGN.md 4.4f's method).
               The robots trot at 0.5 m/s with nothing pending

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_gait.py --out profiles/gait/bench_gait.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mpcqp.controller import BatchedController  # noqa: E402
from mpcqp.estimator import BatchedEstimator  # noqa: E402
from mpcqp.gait import BatchedGaitScheduler  # noqa: E402
from mpcqp.plant import BatchedPlant  # noqa: E402

DEV = "cuda:0"
GAITS = ("standing", "trot10", "pace10")


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


def in_graph(launch, reps):
    """Microseconds per launch of 100 launches captured in one graph."""
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(100):
            launch(s)
    return stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=reps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=20, help="control iterations per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gait needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), horizon=args.horizon, batches={})
    for B in args.batches:
        ctl = BatchedController(B, horizon=args.horizon, robot="aliengo", gait="TROTTING10")
        plant = BatchedPlant(B, controller=ctl)
        sched = BatchedGaitScheduler(B, controller=ctl, gaits=GAITS, initial="trot10")
        est = BatchedEstimator(B, robot="aliengo", controller=ctl)
        eng = ctl.engine
        cur = torch.cuda.current_stream(DEV)
        gyro = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        accel = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        accel[:, 2] = 9.81

        def attitude(stream):
            eng.attitude(est.att_state, gyro, accel, quat=est.quat, gyro_out=est.gyro_corrected,
                         status=est.attitude_status, stream=stream)

        r = {}

        def section(name, launch, check):
            r[name] = stats(per_launch(lambda: launch(cur), n=2000, warm=200, reps=args.reps))
            r[name + "_in_graph"] = in_graph(launch, args.reps)
            r["attitude_beside_" + name] = stats(per_launch(lambda: attitude(cur), n=2000, warm=200, reps=args.reps))
            r["attitude_beside_" + name + "_in_graph"] = in_graph(attitude, args.reps)
            torch.cuda.synchronize()
            assert bool((sched.status == 0).all()) and check(), name

        # idle: nothing pending, the clock advances
        sched.reset()
        section("idle", sched.bind_update(advance=True), lambda: int(sched.switches.sum()) == 0)
        # waiting: every robot asks for pace10 at tick 40 of trot10, aligned and no seam; no advance
        sched.reset()
        sched.tick.fill_(40)
        sched.request("pace10")
        section("waiting", sched.bind_update(advance=False),
                lambda: int(sched.switches.sum()) == 0 and bool((sched.pending == 2).all()) and bool((sched.tick == 40).all()))
        # idle with the iteration output
        sched.reset()
        section("iteration", sched.bind_update(advance=True, iteration=True), lambda: int(sched.switches.sum()) == 0)

        # ---- a control iteration with and without the scheduler, alternated
        sched.reset()
        ctl.reset()
        root, dofs = plant.reset()
        vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
        vb[:, 0] = 0.5
        ctl.set_command(vb, 0.0)
        ibm = ctl.iterations_between_mpc
        ticks = [0]

        def plain():
            ctl.step_fused(ticks[0], None, None, root, dofs)
            plant.step(ctl.tau)
            ticks[0] += 1

        def scheduled():
            sched.update(advance=True)
            ctl.step_fused(None, None, None, root, dofs, mpc_tick=ticks[0] % ibm == 0)
            plant.step(ctl.tau)
            ticks[0] += 1

        for _ in range(200):                  # into the trot
            plain()
        t = dict(plain=[], scheduled=[])
        for _ in range(args.reps):            # each call is warm-up 2 + one timed window
            t["plain"] += per_launch(plain, n=args.window, warm=2, reps=1)
            ctl.tick_count.fill_(ticks[0] - 1)            # the device clock takes over where the host's is
            t["scheduled"] += per_launch(scheduled, n=args.window, warm=2, reps=1)
            assert int(ctl.tick_count[0]) == ticks[0] - 1
        r["step_fused_plant_per_iteration"] = stats(t["plain"])
        r["update_step_fused_plant_per_iteration"] = stats(t["scheduled"])
        r["scheduler_cost_per_iteration_us"] = (r["update_step_fused_plant_per_iteration"]["median_us"]
                                                - r["step_fused_plant_per_iteration"]["median_us"])
        n = int(((plant.status == 0) & (ctl.status == 0) & (sched.status == 0)).sum())
        assert n == B, f"closed loop: {B - n} of {B} robots not OK"
        r["status_ok"] = n
        r["base_height_m"] = [float(plant.root[:, 2].min()), float(plant.root[:, 2].max())]
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
