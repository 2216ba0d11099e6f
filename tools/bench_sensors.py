"""Timing of mpcqp_sensors and mpcqp_push at B = 1024 / 4096 (README, results).
Three questions:

  sensors      the launch alone, eager (back-to-back launches between HIP events: what a caller's
               loop pays per launch, host enqueue included) and 100 launches in a captured graph
               (the device-side cost), with the "mems" preset and with every constant zero (the
               same instructions: a term that is zero is still drawn, only not added), and beside
               each, in the same process, mpcqp_attitude without the trust and mpcqp_plant -- its
               two neighbours in the loop -- and its bandwidth floor: the bytes it moves per robot
               (record 128 B in and the words that change out, 156 B of inputs, 156 B of outputs)
               over the HBM bandwidth of the part
  push         mpcqp_push in a captured graph, at the centre of mass and at a point
  iteration    a control iteration of the closed loop through the sensing chain,
               ``est.update_from_imu; step_fused; plant.step`` against the same with ``sens.update``
               ahead of the estimator, in one process: a fleet of its own stands on the ground
               while the estimator settles for 50 iterations (as tests/test_gpu_disturb.py's loop
               does), then trots at 0.5 m/s on the estimated state; windows of 20 iterations (one
               MPC tick and 19 ticks between two solves) ending in a synchronise, the two
               alternated so drift hits them alike (DESIGN.md 4.4f's method).  Without the stage
               the estimator reads the plant's buffers, with it the stage's

Warm-up before every timed window, the median of the repetitions reported with min and max.
It needs the GPU and does not go through bench.py.  Prints one JSON object and, with --out,
writes it to that file.

  python tools/bench_sensors.py --out profiles/sensors/bench_sensors.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mpcqp.controller import BatchedController  # noqa: E402
from mpcqp.estimator import BatchedEstimator  # noqa: E402
from mpcqp.plant import BatchedPlant  # noqa: E402
from mpcqp.sensors import BatchedSensors  # noqa: E402
import kin_ref  # noqa: E402  (tests/: the standing torques' Jacobians and the standing pose)
import plant_ref  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_US = 8.0e6          # 8 TB/s, the MI355X's nominal HBM3E bandwidth
BYTES_PER_ROBOT = 128 + 13 * 8 + 2 * 156 + 4


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


def loop(B, args):
    """The closed loop through the sensing chain with and without the stage, alternated."""
    ctl = BatchedController(B, horizon=args.horizon, robot="aliengo", gait="TROTTING10")
    plant = BatchedPlant(B, controller=ctl, foot_mass=0.15, substeps=1, ground_z=-0.0255, contact_tol=1e-4)
    par = plant_ref.Params()
    geom = plant.geometry.cpu().numpy()
    root0, _ = plant_ref.stand_pose(B, geom, par)            # the feet on the ground
    plant.reset(height=float(root0[0, 2]))
    est = BatchedEstimator(B, robot="aliengo", controller=ctl, contact_height=par.ground_z)
    sens = BatchedSensors(B, plant=plant, seed=7, preset="mems")
    _, _, Jb = kin_ref.chain(geom, plant.dofs[:, :, 0].cpu().numpy())
    m = float(plant.robot[0, 0])
    stand = np.einsum("blcr,c->blr", Jb, -np.array([0, 0, m * par.gravity / 4])).reshape(B, 12)
    stand = torch.as_tensor(stand.astype(np.float32)).to(DEV).contiguous()
    for it in range(50):                                     # settle: the plant stands while the estimator runs
        plant.step(stand)
        sens.update()
        est.update_from_imu(sens.gyro, sens.accel, sens.dofs, tick=it, touch=sens.touch)
    vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    vb[:, 0] = 0.5
    ctl.set_command(vb, 0.0)
    ticks = [0]

    def plain():
        seen = est.update_from_imu(plant.gyro, plant.accel, plant.dofs, tick=ticks[0], touch=plant.touch)
        ctl.step_fused(ticks[0], None, None, seen, plant.dofs)
        plant.step(ctl.tau)
        ticks[0] += 1

    def sensed():
        sens.update()
        seen = est.update_from_imu(sens.gyro, sens.accel, sens.dofs, tick=ticks[0], touch=sens.touch)
        ctl.step_fused(ticks[0], None, None, seen, sens.dofs)
        plant.step(ctl.tau)
        ticks[0] += 1

    for _ in range(200):                                     # into the trot
        sensed()
    t = dict(plain=[], sensed=[])
    for _ in range(args.reps):                               # each call is one timed window of whole MPC periods
        t["plain"] += per_launch(plain, n=args.window, warm=0, reps=1)
        t["sensed"] += per_launch(sensed, n=args.window, warm=0, reps=1)
    torch.cuda.synchronize()
    r = dict(estimate_step_plant_per_iteration=stats(t["plain"]), sensors_estimate_step_plant_per_iteration=stats(t["sensed"]))
    r["sensors_cost_per_iteration_us"] = (r["sensors_estimate_step_plant_per_iteration"]["median_us"]
                                          - r["estimate_step_plant_per_iteration"]["median_us"])
    n = int(((plant.status == 0) & (ctl.status == 0) & (est.status == 0) & (sens.status == 0)).sum())
    assert n == B, f"closed loop: {B - n} of {B} robots not OK"
    r["status_ok"] = n
    r["base_height_m"] = [float(plant.root[:, 2].min()), float(plant.root[:, 2].max())]
    assert 0.3 < r["base_height_m"][0] and r["base_height_m"][1] < 0.45, r["base_height_m"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=int, default=20, help="control iterations per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sensors needs the GPU: nothing is measured without one")
    res = dict(device=torch.cuda.get_device_name(0), horizon=args.horizon, bytes_per_robot=BYTES_PER_ROBOT, batches={})
    for B in args.batches:
        ctl = BatchedController(B, horizon=args.horizon, robot="aliengo", gait="TROTTING10")
        plant = BatchedPlant(B, controller=ctl)
        est = BatchedEstimator(B, robot="aliengo", controller=ctl)
        sens = BatchedSensors(B, plant=plant, seed=7, preset="mems")
        eng = ctl.engine
        cur = torch.cuda.current_stream(DEV)
        root, dofs = plant.reset()
        gyro = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        accel = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        accel[:, 2] = 9.81
        tau = torch.zeros((B, 12), dtype=torch.float32, device=DEV)

        def attitude(stream):
            eng.attitude(est.att_state, gyro, accel, quat=est.quat, gyro_out=est.gyro_corrected,
                         status=est.attitude_status, stream=stream)

        r = dict(bandwidth_floor_us=B * BYTES_PER_ROBOT / HBM_BYTES_PER_US)

        def section(name, launch):
            r[name] = stats(per_launch(lambda: launch(cur), n=2000, warm=200, reps=args.reps))
            r[name + "_in_graph"] = in_graph(launch, args.reps)
            torch.cuda.synchronize()

        section("sensors_mems", sens.bind_update())
        assert bool((sens.status == 0).all())
        zero = {k: 0 for k in sens.constants if k != "seed"}
        mems = {k: v for k, v in sens.constants.items() if k != "seed"}
        sens.set_constants(**zero)
        section("sensors_zero", sens.bind_update())
        sens.set_constants(**mems)
        section("attitude", attitude)
        plant.reset()
        section("plant_standing", plant.bind_step(tau))
        r["sensors_over_plant_in_graph"] = r["sensors_mems_in_graph"]["median_us"] / r["plant_standing_in_graph"]["median_us"]
        J = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        point = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
        point[:, 0] = 0.1
        r["push_in_graph"] = in_graph(plant.bind_push(J), args.reps)
        r["push_at_point_in_graph"] = in_graph(plant.bind_push(J, point), args.reps)

        r.update(loop(B, args))
        res["batches"][str(B)] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
