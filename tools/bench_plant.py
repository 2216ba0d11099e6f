"""Timing of mpcqp_plant at B = 1024 / 4096 (README, results).  Two questions:

  plant        the launch alone, on the states of the trot: the torques of 100 closed-loop
               iterations are recorded with the record they start from, and every timed window
               restores that record (outside the timing) and replays the 100 launches, which then
               retrace the closed loop exactly -- every robot stays valid and the status is
               asserted OK for all of them after every section.  Back-to-back eager launches
               between HIP events (what a caller's loop pays per launch, host enqueue included)
               and the same 100 launches in a captured graph (the device-side cost), next to the
               bandwidth floor of the bytes the kernel moves per robot (bytes_per_robot: the
               384-byte record in and out, tau, the robot and geometry records in; root_states,
               dof_states, gyro, accel, touch and status out) at 6.3 TB/s achievable.  A robot is
               one quad of lanes running a dependent chain -- the inverse kinematics, a 3 x 3
               inverse and the body update, times substeps, then the kinematics once more for the
               outputs -- so the launch is expected to be bound by latency
  iteration    a control iteration of the closed loop: ``step_fused`` alone (on the state the
               plant last wrote) against ``step_fused; plant.step``, windows of 20 iterations (one
               MPC tick and 19 ticks between two solves) ending in a synchronise, the two
               alternated so drift hits them alike.  The robots trot at 0.5 m/s; the controller's
               and the plant's device state is saved before a ``step_fused``-alone window, which
               advances the planner and the swing generators on a frozen robot, and put back
               after it, so that the ``both`` windows time the trot itself (base_height_m in the
               output shows it)

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_plant.py --out profiles/plant/bench_plant.json
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
from mpcqp.plant import BatchedPlant  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


def bytes_per_robot():
    """read: the record 48 f64, tau 12 f32, the robot record's first 8 f32, the geometry 5 f64;
    written: the record's 43 words, root_states 13, dof_states 24, gyro 3, accel 3, touch 4 f32
    and the status word."""
    return 8 * 48 + 4 * 12 + 4 * 8 + 8 * 5 + 8 * 43 + 4 * (13 + 24 + 3 + 3 + 4) + 4


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
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=20, help="control iterations per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plant needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), horizon=args.horizon, bytes_per_robot=bytes_per_robot(), batches={})
    for B in args.batches:
        ctl = BatchedController(B, horizon=args.horizon, robot="aliengo", gait="TROTTING10")
        plant = BatchedPlant(B, controller=ctl)
        root, dofs = plant.reset()
        vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
        vb[:, 0] = 0.5
        ctl.set_command(vb, 0.0)
        cur = torch.cuda.current_stream(DEV)
        ticks = [0]

        def control():
            ctl.step_fused(ticks[0], None, None, root, dofs)
            ticks[0] += 1

        def both():
            control()
            plant.step(ctl.tau)

        for _ in range(200):                  # into the trot
            both()
        torch.cuda.synchronize()
        assert bool((plant.status == 0).all()) and bool((ctl.status == 0).all())

        def all_ok(what):
            n = int(((plant.status == 0) & (ctl.status == 0)).sum())
            assert n == B, f"{what}: {B - n} of {B} robots not OK"
            return n

        # ---- the launch alone: 100 closed-loop iterations recorded, then replayed from their start
        SEQ = 100
        start = {k: getattr(plant, k).clone() for k in ("state", "root", "dofs")}
        taus = torch.zeros((SEQ, B, 12), dtype=torch.float32, device=DEV)
        for i in range(SEQ):
            control()
            taus[i] = ctl.tau
            plant.step(ctl.tau)
        torch.cuda.synchronize()
        end = plant.state.clone()
        launches = [plant.bind_step(taus[i]) for i in range(SEQ)]

        def restore():
            for k, v in start.items():
                getattr(plant, k).copy_(v)

        def replay_eager():
            for launch in launches:
                launch(cur)

        def timed(fn, warm, reps):
            """Microseconds per launch of one replay of the sequence, the record restored before it."""
            out = []
            for i in range(warm + reps):
                restore()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if i >= warm:
                    out.append(a.elapsed_time(b) * 1e3 / SEQ)
            return out

        r = dict(plant=stats(timed(replay_eager, warm=3, reps=3 * args.reps)))
        assert torch.equal(plant.state, end), "the replay left the closed loop's trajectory"
        r["launch_status_ok"] = all_ok("eager replay")
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for launch in launches:
                launch(s)
        r["plant_in_graph"] = stats(timed(g.replay, warm=3, reps=3 * args.reps))
        assert torch.equal(plant.state, end), "the graph's replay left the closed loop's trajectory"
        r["graph_status_ok"] = all_ok("graph replay")
        floor = bytes_per_robot() * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["plant_in_graph"]["median_us"] / floor
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else \
            "the latency of the launch and of one robot's chain (inverse kinematics, 3 x 3 inverse, body update)"

        # ---- a control iteration with and without the plant, alternated; the loop goes on from `end`
        names = ("plan_state", "swing_mem", "x0", "xref", "contact", "feet", "u0", "tau", "status", "iterations")
        t = dict(control=[], both=[])
        for _ in range(args.reps):            # each call is warm-up 2 + one timed window
            t0 = ticks[0]                      # any 20 consecutive ticks hold one MPC tick
            keep = {k: getattr(ctl, k).clone() for k in names}
            t["control"] += per_launch(control, n=args.window, warm=2, reps=1)
            for k, v in keep.items():          # the planner and the swing generators back where the robot is
                getattr(ctl, k).copy_(v)
            ticks[0] = t0
            t["both"] += per_launch(both, n=args.window, warm=2, reps=1)
        r["step_fused_per_iteration"] = stats(t["control"])
        r["step_fused_plant_per_iteration"] = stats(t["both"])
        r["plant_cost_per_iteration_us"] = (r["step_fused_plant_per_iteration"]["median_us"]
                                            - r["step_fused_per_iteration"]["median_us"])
        r["status_ok"] = all_ok("closed loop")
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
