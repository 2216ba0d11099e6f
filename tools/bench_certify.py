"""Timing of mpcqp_certify at B = 1024 / 4096, N = 10 (README, results), with
mpcqp_predict timed in the same process as the yardstick:

  certify      back-to-back eager launches between HIP events (what a caller's loop pays per
               launch, host enqueue included) and 100 launches in a captured graph (the
               device-side cost), next to the bandwidth floor of the bytes the kernel moves per
               robot (bytes_per_robot: x0, xref, contact, feet, the record and U in; G, the report
               and the status out) at 6.3 TB/s achievable
  predict      the same two figures for mpcqp_predict on the same buffers, alternated with
               certify's so drift hits them alike; certify_over_predict is the ratio of the
               in-graph medians.  A robot's chain in certify is predict's (stage, head, N forward
               scan steps, entries) followed by N backward scan steps, the G entries and the
               foot-step terms, with three wave-level syncs more

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_certify.py --out profiles/certify/bench_certify.json
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
    """read: x0 13, xref 13 N, contact 4 N, feet 12, the record 16 and U 12 N f32; written: G 12 N
    f32, the report 4 f64 and the status word."""
    return 4 * (13 + 13 * N + 4 * N + 12 + 16 + 12 * N) + 4 * 12 * N + 8 * 4 + 4


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def stats(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v))


def per_launch(fn, n, warm, reps=1):
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


def graph_of(launch, cur, n=100):
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(n):
            launch(s)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_certify needs the GPU: nothing is measured without one")
    N = args.horizon
    res = dict(device=torch.cuda.get_device_name(0), horizon=N, bytes_per_robot=bytes_per_robot(N), batches={})
    for B in args.batches:
        bt = make_batch(B, N, seed=B, gaits=("trot10", "pace10", "bound8"), robots=("a1", "aliengo"))
        eng = LinearMpc(horizon=N, robot="a1", device=DEV)
        x0, xref, contact, feet, robot = (dev(bt[k]) for k in ("x0", "xref", "contact", "feet", "robot"))
        f32 = dict(dtype=torch.float32, device=DEV)
        i32 = dict(dtype=torch.int32, device=DEV)
        u0, U = torch.zeros((B, 12), **f32), torch.zeros((B, N, 12), **f32)
        X, G = torch.zeros((B, N, 13), **f32), torch.zeros((B, N, 12), **f32)
        st, it, pst, cst = (torch.zeros((B,), **i32) for _ in range(4))
        prep = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
        crep = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
        cur = torch.cuda.current_stream(DEV)
        solve = eng.bind_solve(B, x0, xref, contact, feet, robot, u0, U, st, it)
        predict = eng.bind_predict(B, x0, xref, contact, feet, robot, U, X, prep, pst)
        certify = eng.bind_certify(B, x0, xref, contact, feet, robot, U, G, crep, cst)
        solve(cur)                 # the U the launches below evaluate
        torch.cuda.synchronize()

        gc, gp = graph_of(certify, cur), graph_of(predict, cur)
        t = dict(certify=[], predict=[], certify_in_graph=[], predict_in_graph=[])
        for _ in range(args.reps):          # alternated; each call is a warm-up and one timed window
            t["certify"] += per_launch(lambda: certify(cur), n=2000, warm=200)
            t["predict"] += per_launch(lambda: predict(cur), n=2000, warm=200)
            t["certify_in_graph"] += [v / 100 for v in per_launch(gc.replay, n=30, warm=5)]
            t["predict_in_graph"] += [v / 100 for v in per_launch(gp.replay, n=30, warm=5)]
        r = {k: stats(v) for k, v in t.items()}
        floor = bytes_per_robot(N) * B / HBM_BYTES_PER_S * 1e6
        r["bandwidth_floor_us"] = floor
        r["graph_over_floor"] = r["certify_in_graph"]["median_us"] / floor
        r["certify_over_predict"] = r["certify_in_graph"]["median_us"] / r["predict_in_graph"]["median_us"]
        r["bound_by"] = "bandwidth" if r["graph_over_floor"] < 2.0 else \
            "the latency of the launch and of one robot's chain (stage, head, two scans of N steps, entries, reduction)"
        rep = crep.cpu().numpy()
        ok = (st.cpu().numpy() == 0) & (cst.cpu().numpy() == 0)
        r["status_ok"] = int(ok.sum())
        r["largest_gap_over_objective"] = float((rep[ok, 1] / np.abs(rep[ok, 0])).max())
        r["lower_le_objective"] = bool((rep[ok, 2] <= rep[ok, 0] + 1e-9 * np.abs(rep[ok, 0])).all())
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
