"""Timing of BatchedController.step_fused (mpcqp_step: the control tick in one C call) against
BatchedController.step (three launches and their host work) at B = 1024 / 4096, TROTTING10,
iterations_between_mpc = 20, N = 10 (README, results).  Per batch size:

  windows      per control iteration, a host clock around a window that ends in a
               synchronise: 200 natural iterations (10 of them MPC ticks), 200 ticks between
               two solves (no MPC tick among them) and 20 MPC ticks, each for ``step``,
               ``step_fused`` with the command set once (set_command) and ``step_fused`` given
               Python lists, the three alternated so drift hits them alike
  launches     back-to-back eager launches between HIP events, host enqueue included: the
               STEP_WHOLE launch, and mpcqp_kinematics, mpcqp_plan and mpcqp_leg_torques each
               on its own -- the three it replaces -- and their sum
  in a graph   100 STEP_WHOLE launches, and 100 times the three launches, captured and
               replayed: the device-side cost without the host (--no-graph skips it)

Warm-up before every timed window, the median of 7 samples reported with min and max.
--step-only measures ``step`` alone; with --package pointing at a checkout of the parent
commit (its library built) that is the parent's figure.  --trace K runs K iterations of
step_fused and exits, for ``rocprofv3 --kernel-trace --stats -- python tools/bench_step.py
--trace 40``.  It needs the GPU and does not go through bench.py.  Prints one JSON object and,
with --out, writes it to that file.

  python tools/bench_step.py --out profiles/step/bench_step.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=200, help="control iterations per timed window")
    ap.add_argument("--package", default=os.path.join(ROOT, "pympc-quadruped_amd"),
                    help="directory holding the mpcqp package to measure")
    ap.add_argument("--step-only", action="store_true", help="measure BatchedController.step alone")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--trace", type=int, default=0, help="run this many step_fused iterations and exit")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = _args()
sys.path[:0] = [ARGS.package, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kin_ref  # noqa: E402
from mpcqp.controller import BatchedController  # noqa: E402

DEV = "cuda:0"
IBM, N = 20, 10
CMD, RATE = [0.5, 0.0, 0.0], 0.1


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def stats(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v))


def window_us(fn, ticks):
    """Microseconds per call of fn(it) over ``ticks``, host clock, ending in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in ticks:
        fn(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / len(ticks)


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


def controller(B):
    return BatchedController(B, horizon=N, robot="a1", gait="TROTTING10", iterations_between_mpc=IBM)


def measure(B, args, res, flush):
    rs, ds = (dev(a[0]) for a in kin_ref.make_states(B, 1, seed=B))
    W = args.window
    windows = dict(natural=list(range(W)), non_mpc=[it for it in range(W + W // (IBM - 1) + 2) if it % IBM][:W],
                   mpc=[IBM * i for i in range(W // 10)])
    r = res["batches"][str(B)] = {}
    paths = {}
    c_step = controller(B)
    paths["step"] = lambda it: c_step.step(it, CMD, RATE, rs, ds)
    if not args.step_only:
        c_set, c_list = controller(B), controller(B)
        c_set.set_command(CMD, RATE)
        paths["step_fused_command_set"] = lambda it: c_set.step_fused(it, None, None, rs, ds)
        paths["step_fused_list_command"] = lambda it: c_list.step_fused(it, CMD, RATE, rs, ds)
    for wname, ticks in windows.items():
        t = {p: [] for p in paths}
        for p, fn in paths.items():          # warm-up: one window each
            window_us(fn, ticks)
        for _ in range(args.reps):           # alternated
            for p, fn in paths.items():
                t[p].append(window_us(fn, ticks))
        r[wname] = {p: stats(v) for p, v in t.items()}
        flush()
    if args.step_only:
        return
    # the runs computed the same thing (the same ticks in the same order on every path)
    torch.cuda.synchronize()
    r["tau_bitwise_equal"] = bool(torch.equal(c_step.tau, c_set.tau) and torch.equal(c_step.tau, c_list.tau))
    r["u0_bitwise_equal"] = bool(torch.equal(c_step.u0, c_set.u0))

    # ---- the launches alone, eager between events
    c, h = controller(B), controller(B)
    vb, yr = c.set_command(CMD, RATE)
    st = torch.cuda.current_stream(DEV)
    eng = c.engine
    whole = eng.bind_step(rs, ds, c.geometry, vb, yr, c.gait, c.plan_state, c.swing_mem, c.x0, c.u0, c.tau)
    kin = dict(root_states=rs, dof_states=ds, feet=h.feet, thighs=h.thighs, pos_feet=h.pos_feet,
               foot_pos_base=h.foot_pos_base, foot_vel_base=h.foot_vel_base, jac=h.jac)
    h.tick_count.fill_(7)

    def f_whole(stream=st):
        whole(0, 7, IBM, stream)

    def f_kin(stream=st):
        h.engine.kinematics(h.geometry, stream=stream, **kin)

    def f_plan(stream=st):
        h.engine.plan(0, h.plan_state, h.x0, vb, yr, root_states=rs, gait=h.gait, iteration=h.iteration,
                      height_des=h.height, xref=h.xref, contact=h.contact, stream=stream)

    def f_leg(stream=st):
        h.engine.leg_torques(h.tick_count, IBM, vb, yr, h.gait, h.thighs, h.pos_feet, h.foot_pos_base,
                             h.foot_vel_base, h.jac, h.u0, h.swing_mem, h.tau, root_states=rs,
                             swing_state=h.swing_state, pos_target=h.pos_target, vel_target=h.vel_target,
                             stream=stream)

    def f_three(stream=st):
        f_kin(stream), f_plan(stream), f_leg(stream)

    eager = {}
    for name, fn in (("whole", f_whole), ("kinematics", f_kin), ("plan", f_plan), ("leg_torques", f_leg),
                     ("three_in_a_row", f_three)):
        eager[name] = stats(per_launch(fn, n=2000, warm=200, reps=args.reps))
    eager["sum_of_three_median_us"] = sum(eager[k]["median_us"] for k in ("kinematics", "plan", "leg_torques"))
    r["launch_eager"] = eager
    flush()
    if args.no_graph:
        return
    # ---- in a graph: the device-side cost (a linear chain of launches on one stream)
    graph = {}
    for name, fn in (("whole", f_whole), ("three_in_a_row", f_three)):
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                fn(s)
        graph[name] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
    r["launch_in_graph"] = graph
    flush()


def main():
    args = ARGS
    if not torch.cuda.is_available():
        sys.exit("bench_step needs the GPU: nothing is measured without one")
    if args.trace:
        B = args.batches[0]
        rs, ds = (dev(a[0]) for a in kin_ref.make_states(B, 1, seed=B))
        ctl = controller(B)
        ctl.set_command(CMD, RATE)
        for it in range(args.trace):
            ctl.step_fused(it, None, None, rs, ds)
        torch.cuda.synchronize()
        print(f"traced {args.trace} iterations of step_fused at B = {B}: {args.trace - (args.trace - 1) // IBM - 1} "
              f"between two solves, {(args.trace - 1) // IBM + 1} MPC ticks")
        return
    res = dict(device=torch.cuda.get_device_name(0), package=os.path.relpath(args.package, ROOT),
               horizon=N, iterations_between_mpc=IBM, gait="TROTTING10", window=args.window, batches={})

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")

    for B in args.batches:
        measure(B, args, res, flush)
    print(json.dumps(res, indent=1))
    flush()


if __name__ == "__main__":
    main()
