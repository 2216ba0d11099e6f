"""Timing of mpcqp_predict at B = 1024 / 4096, N = 10 (README, results).  Two
questions:

  predict      the launch alone: back-to-back eager launches between HIP events (what a caller's
               loop pays per launch, host enqueue included) and 100 launches in a captured graph
               (the device-side cost), next to the bandwidth floor of the bytes the kernel moves
               per robot (bytes_per_robot: x0, xref, contact, feet, the record and U in; X, the
               report and the status out) at 6.3 TB/s achievable.  A robot is one wavefront whose
               lanes 0..11 run a dependent chain of N scan steps through LDS, so the launch is
               expected to be bound by latency, like mpcqp_plan
  tick         an MPC tick: ``solve_raw`` against ``solve_raw; predict_raw`` on the solve's own U,
               windows of 20 ticks ending in a synchronise, the two alternated so drift hits
               them alike

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_predict.py --out profiles/predict/bench_predict.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mpcqp import LinearMpc  # noqa: E402
from mpcqp.synthetic import make_batch  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


def bytes_per_robot(N):
    """read: x0 13, xref 13 N, contact 4 N, feet 12, the record 16 and U 12 N f32; written: X 13 N
    f32, the report 4 f64 and the status word."""
    return 4 * (13 + 13 * N + 4 * N + 12 + 16 + 12 * N) + 4 * 13 * N + 8 * 4 + 4


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
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=20, help="MPC ticks per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_predict needs the GPU: nothing is measured without one")
    N = args.horizon
    res = dict(device=torch.cuda.get_device_name(0), horizon=N, bytes_per_robot=bytes_per_robot(N), batches={})
    for B in args.batches:
        bt = make_batch(B, N, seed=B, gaits=("trot10", "pace10", "bound8"), robots=("a1", "aliengo"))
        eng = LinearMpc(horizon=N, robot="a1", device=DEV)
        x0, xref, contact, feet, robot = (dev(bt[k]) for k in ("x0", "xref", "contact", "feet", "robot"))
        f32 = dict(dtype=torch.float32, device=DEV)
        u0, U, X = torch.zeros((B, 12), **f32), torch.zeros((B, N, 12), **f32), torch.zeros((B, N, 13), **f32)
        st, it = torch.zeros((B,), dtype=torch.int32, device=DEV), torch.zeros((B,), dtype=torch.int32, device=DEV)
        report = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
        pst = torch.zeros((B,), dtype=torch.int32, device=DEV)
        cur = torch.cuda.current_stream(DEV)
        solve = eng.bind_solve(B, x0, xref, contact, feet, robot, u0, U, st, it)
        predict = eng.bind_predict(B, x0, xref, contact, feet, robot, U, X, report, pst)
        solve(cur)                 # the U the launches below evaluate
        torch.cuda.synchronize()

        r = dict(predict=stats(per_launch(lambda: predict(cur), n=2000, warm=200, reps=args.reps)))
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                predict(s)
        r["predict_in_graph"] = stats([v / 100 for v in per_launch(g.replay, n=30, warm=5, reps=args.reps)])
        floor = bytes_per_robot(N) * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["predict_in_graph"]["median_us"] / floor
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else \
            "the latency of the launch and of one robot's chain (stage, head, N scan steps, entries, reduction)"
        rep = report.cpu().numpy()
        ok = (st.cpu().numpy() == 0) & (pst.cpu().numpy() == 0)
        r["status_ok"] = int(ok.sum())
        r["cost_le_cost_free"] = bool((rep[ok, 0] <= rep[ok, 1]).all())
        r["smallest_margin"] = float(rep[ok, 2].min())

        def tick_solve():
            solve(cur)

        def tick_both():
            solve(cur)
            predict(cur)

        t = dict(solve=[], both=[])
        for _ in range(args.reps):          # alternated; each call is warm-up 2 + one timed window
            t["solve"] += per_launch(tick_solve, n=args.window, warm=2, reps=1)
            t["both"] += per_launch(tick_both, n=args.window, warm=2, reps=1)
        r["solve_per_tick"] = stats(t["solve"])
        r["solve_predict_per_tick"] = stats(t["both"])
        r["predict_cost_per_tick_us"] = r["solve_predict_per_tick"]["median_us"] - r["solve_per_tick"]["median_us"]
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
